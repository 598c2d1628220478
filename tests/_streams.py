"""Test-only harness: one entry point on a torch side stream, behind a producer that is still running when the entry is called.

include/resshift_hip.h: "work is enqueued on the caller's hipStream_t".  Torch's side streams are non-blocking - they do not synchronise
with the null stream - so on one of them a launch, memset or copy that went to the null stream, or a host read-back that did not wait for
the caller's stream, runs BEFORE its input exists.  On the null stream (where every other test of the suite runs) the runtime's legacy
ordering hides all of that.  `run_behind_late_producer` makes it visible:

  1. reference: inputs A (seed 0) on the null stream, the entry, synchronise;
  2. spoil: the entry on inputs B (seed 1: same shapes, dtypes and range, finite), synchronise - every engine-internal buffer (arena,
     GroupNorm pools, tickets, FiLM rows, key staging) now holds the data of the wrong inputs, and everything that grows or is cached on
     first use has grown and is cached;
  3. side stream: buffers filled with B; a producer on the stream - a chain of dependent matrix products whose last link gates a copy of A
     into the buffers, so A exists only when the whole chain has run; an event behind it; the entry; the result cloned on the stream;
  4. verdict: the result equals the reference bit for bit; the event was still pending when the entry was called (else the case proved
     nothing and FAILS); with must_not_block it was still pending when the entry returned.

The producer: LINKS links of tanh(c @ m) on N x N fp32 matrices (values stay in [-1, 1]: finite whatever happens), each dependent on the
one before - a real dependency chain, no spinning kernel.
Its length was set on the MI355X, from 4 links (4.3 ms between two events) upwards: one link takes 0.94 ms, 24 links 22.4 ms, LINKS =
40 links 37.4 ms.  The slowest-to-enqueue ASYNC entry is Engine.sample, seeded, at B = 70 (begin + 4 steps + end of the tiny case, dry sizing
pass included): 2.04 .. 2.25 ms on the host, and 20 consecutive harness runs of it kept both flags - the producer outlasts it 17 times
over, which leaves room for a loaded host.  tests/test_streams_gpu.py prints both figures on every run.
(The first use of a torch kernel loads its code object on the host, 20 ms and more: the harness therefore runs one link and the gated
copies once on the null stream before it goes to the side stream - without that the first case of a process found its producer over.)
"""
import torch

N = 4096
LINKS = 40
PRODUCER_MS = 37.4            # measured: the chain between two events
SLOWEST_ENQUEUE_MS = 2.25     # measured: host time of Engine.sample, seeded, B = 70, the largest of 20 runs

_CHAIN = {}


_SIDE = {}


def side_stream(dev, k=0):
    """side stream k (0 or 1) of the device, made once: with the null stream at most three streams are ever in use"""
    assert k in (0, 1)
    if (dev, k) not in _SIDE:
        _SIDE[(dev, k)] = torch.cuda.Stream(dev)
    return _SIDE[(dev, k)]


def _chain_operands(dev):
    if dev not in _CHAIN:
        g = torch.Generator().manual_seed(99)
        c = (torch.rand(N, N, generator=g) * 2 - 1).to(dev)
        m = ((torch.rand(N, N, generator=g) * 2 - 1) / N ** 0.5).to(dev)
        torch.tanh(c @ m)           # (the BLAS library's first call picks its kernel on the host: not inside a measured region)
        torch.cuda.synchronize(dev)
        _CHAIN[dev] = (c, m)
    return _CHAIN[dev]


def enqueue_chain(dev, links=None):
    """the dependency chain on the current stream; returns a 0-dim bool tensor that is true - and known only when the chain has run"""
    c, m = _chain_operands(dev)
    for _ in range(LINKS if links is None else links):
        c = torch.tanh(c @ m)
    return c.abs().max() <= 1.0


def chain_ms(dev, links=None):
    """milliseconds of the chain on the current stream, between two events"""
    _chain_operands(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    enqueue_chain(dev, links)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def leaves(tree, path=""):
    """[(path, leaf)] of a result or an input tree: tensors, bytes, numbers, in lists / tuples / dicts"""
    if isinstance(tree, dict):
        return [p for k in tree for p in leaves(tree[k], f"{path}[{k!r}]")]
    if isinstance(tree, (list, tuple)):
        return [p for i, v in enumerate(tree) for p in leaves(v, f"{path}[{i}]")]
    return [(path, tree)]


def tree_map(fn, tree):
    if isinstance(tree, dict):
        return {k: tree_map(fn, v) for k, v in tree.items()}
    if isinstance(tree, (list, tuple)):
        return type(tree)(tree_map(fn, v) for v in tree)
    return fn(tree)


def assert_equal_trees(got, want, what):
    lg, lw = leaves(got), leaves(want)
    assert [p for p, _ in lg] == [p for p, _ in lw], (what, [p for p, _ in lg], [p for p, _ in lw])
    for (p, a), (_, b) in zip(lg, lw):
        if isinstance(b, torch.Tensor):
            assert isinstance(a, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype, (what, p)
            if not torch.equal(a, b):
                differ = int((a != b).sum())
                raise AssertionError(f"{what}: result{p} on the side stream differs from the null-stream result in {differ} of {b.numel()} elements")
        else:
            assert a == b, f"{what}: result{p} on the side stream differs from the null-stream result"


def _check_inputs(a, b, what):
    for (p, ta), (_, tb) in zip(leaves(a), leaves(b)):
        assert isinstance(ta, torch.Tensor) and ta.is_cuda, (what, p, "inputs are device tensors; host arguments belong in the call")
        assert ta.shape == tb.shape and ta.dtype == tb.dtype, (what, p)
        if ta.is_floating_point():
            assert bool(torch.isfinite(tb).all()), (what, p, "the poison must be finite")


def run_behind_late_producer(make_inputs, call, *, must_not_block, what="", stream=None, report=None):
    """See the module docstring.  make_inputs(seed) -> a tree of device tensors (seed 0: the inputs, seed 1: the poison); call(inputs) -> a
    tree of tensors / bytes / numbers (an in-place entry returns the inputs it has written).  Raises AssertionError on a mismatch, on a
    producer that was over before the call, and - must_not_block - on an entry that returned only after the producer.  `report`: a dict
    that receives the host milliseconds of the side-stream call."""
    import time

    dev = torch.device("cuda", torch.cuda.current_device())
    assert torch.cuda.current_stream(dev) == torch.cuda.default_stream(dev), "the harness starts on the null stream"
    a = make_inputs(0)
    b = make_inputs(1)
    _check_inputs(a, b, what)
    want = tree_map(lambda t: t.clone() if isinstance(t, torch.Tensor) else t, call(tree_map(torch.clone, a)))
    torch.cuda.synchronize(dev)
    call(tree_map(torch.clone, b))                                  # spoil
    # (one link of the producer and the gated copies, here on the null stream: the first use of a torch kernel loads its code object on the
    # host, which on the side stream would happen between the chain and the call and let the chain run out)
    gate = enqueue_chain(dev, 1)
    for (_, buf), (_, src) in zip(leaves(tree_map(torch.clone, b)), leaves(a)):
        buf.copy_(torch.where(gate, src, buf))
    torch.cuda.synchronize(dev)
    s = side_stream(dev) if stream is None else stream
    with torch.cuda.stream(s):
        bufs = tree_map(torch.clone, b)                             # the poison
        gate = enqueue_chain(dev)
        for (_, buf), (_, src) in zip(leaves(bufs), leaves(a)):
            buf.copy_(torch.where(gate, src, buf))                  # A, data-dependent on the last link
        e = torch.cuda.Event()
        e.record(s)
        pending_before = not e.query()
        t0 = time.perf_counter()
        out = call(bufs)
        host_ms = (time.perf_counter() - t0) * 1e3
        pending_after = not e.query()
        got = tree_map(lambda t: t.clone() if isinstance(t, torch.Tensor) else t, out)
        s.synchronize()
    if report is not None:
        report["host_ms"] = host_ms
    torch.cuda.synchronize(dev)
    assert pending_before, f"{what}: the producer was over before the entry was called - the case proved nothing"
    assert_equal_trees(got, want, what)
    if must_not_block:
        assert pending_after, f"{what}: the entry returned only after its producer had run ({host_ms:.1f} ms on the host): it blocks"
    return got

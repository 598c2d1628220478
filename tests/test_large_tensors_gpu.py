"""Every kernel family on tensors past 2^31 bytes, every image of the result against float64; the per-operand size limit at its boundary.

The rest of the suite stops at 1 GiB per operand.  Seven kernel families reach their operands through a buffer descriptor plus a 32-bit
per-lane byte offset and refuse operands of RS_BUFFER_BYTES_LIMIT (0xF0000000) bytes or more; the others use 64-bit pointer arithmetic.
Between 2^31 bytes and the limit every `unsigned` / `int` / `long long` conversion on an address path matters, and nothing measured it.

Operands (tests/_large.py): P = 3 distinct images repeated along the batch, residuals drawn from another seed; the reference is float64 of
the three images (convs: `reference` of tests/test_conv_plan_gpu.py on the device; the rest: the restatements of tests/test_ops_gpu.py), and
EVERY image b of the result is compared with ref[b % 3], in chunks, at the tolerance tests/test_ops_gpu.py has for that kernel and storage.
Rows that go through ops.conv2d reach the byte counts with few pixels through wide rows (ld0 / ldy / ldres, the padding of the sources LOUD,
that of y a bit pattern that must survive, one more image of it behind the result); tests/test_large_tensors_cpu.py holds that the wide
rows leave the plan as it is, and that no operand's period divides 2^31 or 2^32 bytes.  The halo, Winograd, attention, MLP, GroupNorm
and layout wrappers take dense tensors only: there the pixels make the bytes.

Engine level: rs_vq_encode of the shipped realsr autoencoder at B = 66 in split storage (first-level tensors of 2.06 GiB, image 64 starts
at byte 2^31), z of every image against the fp32 oracle under the tolerance of test_autoencoder_vs_oracle: 2.5e-6 of 2e-5, the nearest code
the same at every position.  rs_vq_decode at B = 33 (3.2e-6 of 2e-5) puts the halo kernel's folded-shortcut source (sx, 2.06 GiB: dec.up.0.block.0) past
2^31 bytes, which no op-level entry can: the launch is found in the profiled pass, every image is compared with the oracle.

Boundary: for igemm2, igemm3, the halo kernel, igemm_split, wino and both fused attention kernels, the largest batch whose x stays below the
limit runs and is compared like the rest; one more image is refused with the named text (operand, bytes, limit, largest batch) and nothing
is launched - the result tensor keeps the bit pattern it was filled with.

Each test frees the device memory before and after, prints its peak and holds it under 16 GiB; with less than that free it skips, loudly.

Measured on the MI355X: all 31 cases pass in 18.6 s (the file's whole pytest run).  The two engine cases take 3.3 s and 4.3 s, the CPU
oracle of their three images included, the fp32 layout case 1.2 s, no other case 0.6 s - the tensors are large, the arithmetic is not.
For scale: tests/test_ops_gpu.py, test_conv_plan_gpu.py and test_ops_regimes_gpu.py together take 23 s; the GPU suite before this file was
not timed in one piece - its first 758 of 1401 tests (through tests/test_engine_gpu.py's tiled-path cases) take 1000 s.  Worst error against its tolerance: 0.22 (igemm3 fp16, 4.3e-4 of 2e-3); split storage stays below 0.2
(halo 5.7e-7 of 3e-6); peaks 2.4 .. 12.2 GiB (DESIGN section 4.6 has the table).  No kernel defect was found.

Three mutants, one scratch build each, never committed, each aliasing an address INSIDE its tensor.  "Before" is a SUBSET of the existing
suite, the three files that launch these kernels one at a time - tests/test_ops_gpu.py, tests/test_conv_plan_gpu.py and
tests/test_ops_regimes_gpu.py: 853 passed / 19 skipped with every mutant, as without; the block, engine and sampler files were not run
on the mutants:
(1) igemm2's set_tap clears bit 31 of the pixel byte offset.  Fails test_conv_past_2g[igemm2-f16], [igemm2-f32] and
    test_conv_limit_boundary[igemm2-f16]; nothing else.
(2) gn_stats_kernel forms the image base as a 32-bit product that loses bit 31 (an `int` product, with the sign bit masked so that the read
    stays inside the tensor).  Fails test_groupnorm_past_2g_elements[f16] (image 2048 alone reads image 0's statistics: the three base images
    differ in scale and offset so that this shows at 2e-3) and [split].  (A failed case keeps its 8 GiB tensor alive in its traceback, which
    made the next test's 16 GiB assertion fire as well.)
(3) igemm_split's epilogue.  As specified - rs_out_m(p, m) * p.ldy truncated to 32 bits - the mutant cannot show below 16 GiB of y: the
    product counts ELEMENTS, and 2^32 of them are 16 GiB in split storage (the largest product here is 5.5e8).  Planted instead: the row's
    BYTE offset loses bit 31 ((rs_out_m(p, m) * p.ldy * 2) & 0x3fffffff in halfs).  Fails test_conv_past_2g[split-1x1] and [split-3x3s2];
    the split-K row's y is written by the reduce kernel, the boundary row's y is small.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import _conv_classes as CC
import _large as LG
from test_conv_plan_gpu import reference
from test_ops_gpu import TOL, TOL_SPLIT, _window_attention_reference

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(bool(CC.planner_env()), reason=f"planner knobs set in the environment: {CC.planner_env()}")]
torch.set_grad_enabled(False)
P = LG.P
# the figures of tests/test_ops_gpu.py, by test: test_conv_direct, test_groupnorm / test_groupnorm_split, test_window_attention_fused_qkv(_split),
# test_swin_mlp_fused(_split), test_conv3x3_halo_split_storage, test_conv3x3_wino_split_storage, the statistics slabs of the halo / wino tests
TOL_DIRECT, TOL_GN_F16, TOL_GN_SPLIT, TOL_ATTN_F16, TOL_ATTN_SPLIT = 2e-5, 2e-3, 5e-6, 3e-3, 5e-6
TOL_MLP_F16, TOL_MLP_SPLIT, TOL_HALO_SPLIT, TOL_WINO, TOL_STATS = 2e-3, 3e-6, 3e-6, 6e-6, 1e-3


@pytest.fixture(autouse=True)
def _device_memory(gpu):
    LG.free()
    have = torch.cuda.mem_get_info()[0]
    if have < LG.PEAK_BYTES:
        print(f"\n[large] SKIPPED: {have / 2 ** 30:.1f} GiB of device memory free, the test may use up to {LG.PEAK_BYTES / 2 ** 30:.0f} GiB")
        pytest.skip(f"only {have / 2 ** 30:.1f} GiB of device memory free")
    torch.cuda.reset_peak_memory_stats()
    yield
    peak = torch.cuda.max_memory_allocated()
    print(f"\n[large] peak device memory {peak / 2 ** 30:.2f} GiB")
    LG.free()
    assert peak < LG.PEAK_BYTES, f"peak device memory {peak / 2 ** 30:.2f} GiB"


def _conv_tol(L):
    if L.in_prec == CC.SPLIT:
        return TOL_SPLIT
    return TOL[torch.float16] if L.out_prec == CC.F16 else TOL[torch.float32]


def _conv_operands(c):
    """P base images of the case's layer: x, w, b and (another seed) the residual, fp32 on the CPU, rounded where the storage rounds"""
    L = c.L
    Ho, Wo = CC.out_hw(L)
    g, gr = torch.Generator().manual_seed(LG.seed_of(c.name, tuple(L))), torch.Generator().manual_seed(LG.seed_of(c.name, "residual"))
    x = torch.randn(P, L.Cin, L.H, L.W, generator=g)
    w = torch.randn(L.Cout, L.Cin, L.k, L.k, generator=g) / math.sqrt(L.Cin * L.k * L.k)
    b = torch.randn(L.Cout, generator=g)
    r = torch.randn(P, L.Cout, Ho, Wo, generator=gr) if L.res else None
    if L.in_prec == CC.F16:
        x, w = x.half().float(), w.half().float()
    if r is not None and L.out_prec == CC.F16:
        r = r.half().float()
    return x, w, b, r


def _run_conv(c, dev, B=None, refused=False):
    """one ops.conv2d launch of a ConvCase at batch B: (plan, error over all images, padding and tail image intact); refused: the call
    must raise, and (None, message, result tensor untouched) comes back"""
    from resshift_amd import ops

    L = c.L if B is None else c.L._replace(B=B)
    B = L.B
    ld0, ldy, ldres = c.ld
    Ho, Wo = CC.out_hw(L)
    x, w, b, r = _conv_operands(c)
    C0 = L.Cin - c.C1
    xd = LG.tile(LG.store(x[:, :C0], L.in_prec, dev, ld0), B)
    x1d = LG.tile(LG.store(x[:, C0:], L.in_prec, dev), B) if c.C1 else None
    rd = LG.tile(LG.store(r, L.out_prec, dev, ldres), B) if r is not None else None
    backing = LG.sentinel_fill(torch.empty(B + 1, Ho, Wo, ldy, device=dev, dtype=ops._dt(L.out_prec)))
    kw = dict(x1=x1d, res=rd, stride=L.stride, pad=(L.k // 2, L.k // 2), up=L.up, out_prec=L.out_prec, ld=c.ld, return_plan=True, out=backing[:B],
              force_direct=c.kernel == "CK_NONE")
    if refused:
        with pytest.raises(RuntimeError) as e:
            ops.conv2d(xd, w, b, **kw)
        torch.cuda.synchronize()
        return None, str(e.value), LG.sentinel_intact(backing)
    y, plan = ops.conv2d(xd, w, b, **kw)
    torch.cuda.synchronize()
    del xd, x1d, rd
    ref = reference(L._replace(B=P), x, w, b, r, torch.float64, dev)
    err = LG.rel_err_all_images(lambda b0, b1: LG.load(y[b0:b1], L.out_prec, L.Cout), ref, B)
    intact = LG.sentinel_intact(backing[:B], L.Cout) and LG.sentinel_intact(backing[B:])
    return CC.Plan(*plan), err, intact


@pytest.mark.parametrize("c", LG.CONV_CASES, ids=[c.name for c in LG.CONV_CASES])
def test_conv_past_2g(gpu, c):
    per = LG.conv_bytes(c)
    for o in c.big.split():
        assert LG.G31 < c.L.B * per[o] < LG.LIMIT or c.kernel in ("CK_IGEMM", "CK_NONE"), (o, c.L.B * per[o])
        assert c.L.B * per[o] > LG.G31
    plan, err, intact = _run_conv(c, gpu)
    print(f"\n[large] conv {c.name}: " + ", ".join(f"{o} {c.L.B * per[o] / 2 ** 30:.3f} GiB" for o in ("x", "y", "res") if per[o])
          + f", plan {tuple(plan)}, err {err:.3e} (tol {_conv_tol(c.L) if c.kernel != 'CK_NONE' else TOL_DIRECT:.0e}), padding intact: {intact}")
    assert plan.kernel == c.kernel and (plan.splitk > 1) == c.sk, plan
    assert intact, "the launch wrote into y's padding columns or behind its last image"
    assert err <= (TOL_DIRECT if c.kernel == "CK_NONE" else _conv_tol(c.L)), err


@pytest.mark.parametrize("c", LG.BOUNDARY_CONV, ids=[c.name for c in LG.BOUNDARY_CONV])
def test_conv_limit_boundary(gpu, c):
    """the largest batch whose x0 stays below the limit runs right; one more image is refused by name and launches nothing"""
    from resshift_amd import ops  # noqa: F401

    per = LG.conv_bytes(c)["x"]
    assert c.L.B * per < LG.LIMIT <= (c.L.B + 1) * per and LG.LIMIT - c.L.B * per <= per
    plan, err, intact = _run_conv(c, gpu)
    print(f"\n[large] boundary {c.name}: x {c.L.B * per} bytes accepted, plan {tuple(plan)}, err {err:.3e}, padding intact: {intact}")
    assert plan.kernel == c.kernel and intact and err <= _conv_tol(c.L), (plan, err, intact)
    LG.free()
    _, text, untouched = _run_conv(c, gpu, B=c.L.B + 1, refused=True)
    print(f"[large] boundary {c.name}: x {(c.L.B + 1) * per} bytes refused: {text}")
    _assert_named(text, "x0", (c.L.B + 1) * per, c.L.B)
    assert untouched, "a refused launch wrote into its result tensor"


def _assert_named(text, operand, nbytes, fits):
    assert f"operand {operand} " in text and f"is {nbytes} bytes" in text and str(LG.LIMIT) in text and text.rstrip().endswith(f"the largest batch that fits is {fits}"), text


# ---------------------------------------------------------------- halo and Winograd kernels: input transform, statistics, residual
def _fused_conv_case(dev, shape, wino, B=None, refused=False):
    from resshift_amd import ops

    B0, H, W, Cin, Cout, split = shape
    B = B0 if B is None else B
    prec = CC.SPLIT if split else CC.F16
    g, gr = torch.Generator().manual_seed(LG.seed_of("fused conv", shape, wino)), torch.Generator().manual_seed(LG.seed_of("fused conv residual", shape, wino))
    x = torch.randn(P, Cin, H, W, generator=g) * 1.5 + 0.2
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    bias = torch.randn(Cout, generator=g)
    a, d = torch.randn(P, Cin, generator=g) * 0.3 + 1.0, torch.randn(P, Cin, generator=g) * 0.5
    r = torch.randn(P, Cout, H, W, generator=gr)
    xd = LG.tile(LG.store(x, prec, dev), B)
    coef = LG.tile(torch.stack([a, d], 1).contiguous().to(dev), B).contiguous()
    if refused:   # (the Winograd boundary: no residual, the result tensor pre-filled)
        out = LG.sentinel_fill(torch.empty(B, H, W, Cout, device=dev, dtype=torch.int32))
        with pytest.raises(RuntimeError) as e:
            ops.conv3x3_wino(xd, w, bias, coef=coef, act_in=2, out=out)
        torch.cuda.synchronize()
        return str(e.value), LG.sentinel_intact(out)
    rd = LG.tile(LG.store(r, prec, dev), B)
    fn = ops.conv3x3_wino if wino else ops.conv3x3_halo
    y, st = fn(xd, w, bias, coef=coef, act_in=2, res=rd, want_stats=True)
    torch.cuda.synchronize()
    del xd, rd
    L = CC.Layer(prec, prec, P, H, W, Cin, Cout, 3, 1, 1, True)
    ad, dd = a.to(dev)[:, :, None, None], d.to(dev)[:, :, None, None]
    if split:
        xr, wr = F.silu(x.to(dev).double() * ad.double() + dd.double()), w
    else:   # (rounded where the kernel rounds, as test_conv3x3_halo_with_fused_groupnorm_affine has it)
        xr, wr, r = F.silu(x.to(dev).half().float() * ad + dd).half().double(), w.half().float(), r.half().float()
    ref = reference(L, xr, wr, bias, r if L.res else None, torch.float64, dev)
    err = LG.rel_err_all_images(lambda b0, b1: LG.load(y[b0:b1], prec, Cout), ref, B)
    serr = LG.stats_rel_err(st, lambda b0, b1: LG.load(y[b0:b1], prec, Cout), B)
    return err, serr


@pytest.mark.parametrize("name,shape,wino,tol", [("halo-f16", LG.HALO_F16, False, TOL[torch.float16]), ("halo-split", LG.HALO_SPLIT, False, TOL_HALO_SPLIT),
                                                 ("wino-split", LG.WINO_SPLIT, True, TOL_WINO)], ids=["halo-f16", "halo-split", "wino-split"])
def test_fused_conv_past_2g(gpu, name, shape, wino, tol):
    """ops.conv3x3_halo (raises unless the plan is CK_HALO or CK_HALO_SEG; ops.conv_plan says CK_HALO) / ops.conv3x3_wino (raises unless the
    plan is CK_WINO): GroupNorm affine + SiLU on the input, the
    statistics slabs of the stored result, a residual; x, y and the residual each between 2^31 bytes and the limit"""
    nbytes = shape[0] * LG.dense_bytes(shape, shape[3], 4 if shape[5] else 2)
    assert LG.G31 < nbytes < LG.LIMIT and shape[3] == shape[4]
    if not wino:   # (ops.conv_plan cannot ask for the Winograd kernel - its plan needs packed weights; ops.conv3x3_wino raises unless it ran)
        assert LG.dense_halo_plan(shape).kernel == "CK_HALO", LG.dense_halo_plan(shape)
    err, serr = _fused_conv_case(gpu, shape, wino)
    print(f"\n[large] {name}: x = y = res {nbytes / 2 ** 30:.3f} GiB, err {err:.3e} (tol {tol:.0e}), statistics {serr:.3e} (tol {TOL_STATS:.0e})")
    assert err <= tol and serr < TOL_STATS, (err, serr)


def test_wino_limit_boundary(gpu):
    shape = LG.WINO_BOUNDARY
    per = LG.dense_bytes(shape, shape[3], 4)
    assert shape[0] * per < LG.LIMIT == (shape[0] + 1) * per
    err, serr = _fused_conv_case(gpu, shape, True, B=shape[0])
    print(f"\n[large] boundary wino: x {shape[0] * per} bytes accepted, err {err:.3e}, statistics {serr:.3e}")
    assert err <= TOL_WINO and serr < TOL_STATS, (err, serr)
    LG.free()
    text, untouched = _fused_conv_case(gpu, shape, True, B=shape[0] + 1, refused=True)
    print(f"[large] boundary wino: x {(shape[0] + 1) * per} bytes refused: {text}")
    _assert_named(text, "x0", (shape[0] + 1) * per, shape[0])
    assert untouched, "a refused launch wrote into its result tensor"


# ---------------------------------------------------------------- fused qkv + window attention + projection + shortcut
def _attention_case(dev, shape, split, B=None, refused=False):
    from resshift_amd import ops

    B0, H, W = shape
    B = B0 if B is None else B
    heads, E, shift = 6, 192, 4
    prec = CC.SPLIT if split else CC.F16
    g, gr = torch.Generator().manual_seed(LG.seed_of("attention", shape, split)), torch.Generator().manual_seed(LG.seed_of("attention residual", shape, split))
    x = torch.randn(P, E, H, W, generator=g)
    wqkv, bqkv = torch.randn(3 * E, E, generator=g) / math.sqrt(E), torch.randn(3 * E, generator=g) * 0.2
    table = torch.randn(225, heads, generator=g) * 0.5
    wproj, bproj = torch.randn(E, E, generator=g) / math.sqrt(E), torch.randn(E, generator=g) * 0.2
    res = torch.randn(P, E, H, W, generator=gr)
    if not split:
        x, wqkv, wproj, res = x.half().float(), wqkv.half(), wproj.half(), res.half().float()
    xd, rd = LG.tile(LG.store(x, prec, dev), B), LG.tile(LG.store(res, prec, dev), B)
    fn = ops.window_attention_qkv_split if split else ops.window_attention_qkv
    if refused:
        out = LG.sentinel_fill(torch.empty(B, H, W, E, device=dev, dtype=xd.dtype))
        with pytest.raises(RuntimeError) as e:
            fn(xd, wqkv, bqkv, table, heads, shift, wproj=wproj, bproj=bproj, res=rd, out=out)
        torch.cuda.synchronize()
        return str(e.value), LG.sentinel_intact(out)
    y = fn(xd, wqkv, bqkv, table, heads, shift, wproj=wproj, bproj=bproj, res=rd)
    torch.cuda.synchronize()
    del xd, rd
    # the restatement of tests/test_ops_gpu.py (it builds its mask on the CPU: three images there, in float64; fp16 storage rounds qkv and
    # the attention result to fp16 as the kernel's operands are)
    rnd = (lambda t: t) if split else (lambda t: t.half().double())
    qkv = torch.einsum("bchw,oc->bohw", x.double(), wqkv.double()) + bqkv.double()[None, :, None, None]
    attn = _window_attention_reference(rnd(qkv), table.double(), heads, shift)
    ref = (torch.einsum("bchw,oc->bohw", rnd(attn), wproj.double()) + bproj.double()[None, :, None, None] + res.double()).to(dev)
    return LG.rel_err_all_images(lambda b0, b1: LG.load(y[b0:b1], prec, E), ref, B)


@pytest.mark.parametrize("split", [False, True], ids=["f16", "split"])
def test_window_attention_qkv_past_2g(gpu, split):
    shape = LG.ATTN_SPLIT if split else LG.ATTN_F16
    nbytes = shape[0] * LG.dense_bytes(shape, 192, 4 if split else 2)
    assert LG.G31 < nbytes < LG.LIMIT
    err = _attention_case(gpu, shape, split)
    tol = TOL_ATTN_SPLIT if split else TOL_ATTN_F16
    print(f"\n[large] window_attention_qkv{'_split' if split else ''}: x = res = out {nbytes / 2 ** 30:.3f} GiB, err {err:.3e} (tol {tol:.0e})")
    assert err <= tol, err


@pytest.mark.parametrize("split", [False, True], ids=["f16", "split"])
def test_window_attention_qkv_limit_boundary(gpu, split):
    shape = LG.ATTN_SPLIT_BOUNDARY if split else LG.ATTN_F16_BOUNDARY
    per = LG.dense_bytes(shape, 192, 4 if split else 2)
    assert shape[0] * per < LG.LIMIT == (shape[0] + 1) * per
    err = _attention_case(gpu, shape, split)
    print(f"\n[large] boundary window_attention_qkv{'_split' if split else ''}: x {shape[0] * per} bytes accepted, err {err:.3e}")
    assert err <= (TOL_ATTN_SPLIT if split else TOL_ATTN_F16), err
    LG.free()
    text, untouched = _attention_case(gpu, shape, split, B=shape[0] + 1, refused=True)
    print(f"[large] boundary window_attention_qkv{'_split' if split else ''}: x {(shape[0] + 1) * per} bytes refused: {text}")
    _assert_named(text, "x", (shape[0] + 1) * per, shape[0])
    assert untouched, "a refused launch wrote into its result tensor"


# ---------------------------------------------------------------- fused Swin MLP
@pytest.mark.parametrize("split", [False, True], ids=["f16", "split"])
def test_swin_mlp_past_2g(gpu, split):
    from resshift_amd import ops

    B, T = LG.MLP_SPLIT if split else LG.MLP_F16
    E, HD = 192, 768
    assert B * T * E * (4 if split else 2) > LG.G31
    g, gr = torch.Generator().manual_seed(LG.seed_of("mlp", split)), torch.Generator().manual_seed(LG.seed_of("mlp residual", split))
    x = torch.randn(P, T, E, generator=g)
    w1, w2 = torch.randn(HD, E, generator=g) / math.sqrt(E), torch.randn(E, HD, generator=g) / math.sqrt(HD)
    b1, b2 = torch.randn(HD, generator=g) * 0.3, torch.randn(E, generator=g) * 0.3
    res = torch.randn(P, T, E, generator=gr)
    if split:
        xd, rd = LG.tile(ops.convert(x.to(gpu), ops.SPLIT), B), LG.tile(ops.convert(res.to(gpu), ops.SPLIT), B)
    else:
        x, w1, w2, res = x.half().float(), w1.half().float(), w2.half().float(), res.half().float()
        xd, rd = LG.tile(x.to(gpu).half(), B), LG.tile(res.to(gpu).half(), B)
    y = ops.swin_mlp(xd.view(B * T, E), w1, b1, w2, b2, rd.view(B * T, E)).view(B, T, E)
    torch.cuda.synchronize()
    del xd, rd
    d = lambda t: t.to(gpu, torch.float64)   # noqa: E731
    h = F.gelu(d(x) @ d(w1).t() + d(b1))
    if not split:
        h = h.half().double()   # (the hidden activations are stored as fp16, test_swin_mlp_fused)
    ref = h @ d(w2).t() + d(b2) + d(res)
    err = LG.rel_err_all_images(lambda b0, b1: ops.convert(y[b0:b1].contiguous(), ops.F32) if split else y[b0:b1], ref, B, chunk=16 * P)
    tol = TOL_MLP_SPLIT if split else TOL_MLP_F16
    print(f"\n[large] swin_mlp{'_split' if split else ''}: x = res = y {B * T * E * (4 if split else 2) / 2 ** 30:.3f} GiB, err {err:.3e} (tol {tol:.0e})")
    assert err <= tol, err


# ---------------------------------------------------------------- GroupNorm, more than 2^31 elements
@pytest.mark.parametrize("split", [False, True], ids=["f16", "split"])
def test_groupnorm_past_2g_elements(gpu, split):
    """statistics pass + apply pass (the plane has more than 256 pixels).  In place: the apply pass is elementwise and starts when the
    statistics pass has ended - two split-storage tensors of 2^31 elements would be 16 GiB"""
    from resshift_amd import ops

    B, H, W, C = LG.GN_SHAPE
    assert B * H * W * C > LG.G31 and H * W > 256
    g = torch.Generator().manual_seed(LG.seed_of("groupnorm", split))
    # (the three images differ in scale and offset: statistics taken from another image of the period must show at the fp16 tolerance too)
    x = torch.randn(P, C, H, W, generator=g) * torch.tensor([1.7, 0.6, 3.1]).view(P, 1, 1, 1) + torch.tensor([0.3, -0.1, 0.5]).view(P, 1, 1, 1)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    film = torch.randn(2 * C, generator=g) * 0.5
    if not split:
        x = x.half().float()
    xd = LG.tile(LG.store(x, CC.SPLIT if split else CC.F16, gpu), B)
    y = ops.groupnorm(xd, gamma, beta, 1e-5, act=2, film=film.to(gpu), out=xd)
    torch.cuda.synchronize()
    ref = F.group_norm(x.to(gpu).double(), 32, gamma.to(gpu).double(), beta.to(gpu).double(), 1e-5)
    ref = F.silu(ref * (1 + film[:C].to(gpu).double().view(1, C, 1, 1)) + film[C:].to(gpu).double().view(1, C, 1, 1))
    err = LG.rel_err_all_images(lambda b0, b1: LG.load(y[b0:b1], CC.SPLIT if split else CC.F16, C), ref, B, chunk=16 * P)
    tol = TOL_GN_SPLIT if split else TOL_GN_F16
    print(f"\n[large] groupnorm{'_split' if split else ''}: {B * H * W * C} elements, err {err:.3e} (tol {tol:.0e})")
    assert err <= tol, err


# ---------------------------------------------------------------- storage and layout kernels, more than 2^31 elements, exact
def test_convert_past_2g_elements(gpu):
    from resshift_amd import ops

    B, H, W, C = LG.ELEMENTWISE_SHAPE
    assert B * H * W * C > LG.G31
    g = torch.Generator().manual_seed(LG.seed_of("convert"))
    src = LG.tile((torch.randn(P, H, W, C, generator=g) * 3).to(gpu).half(), B)
    dst = ops.convert(src, ops.F32)
    torch.cuda.synchronize()
    assert dst.shape == src.shape and dst.dtype == torch.float32
    assert LG.equal_all_images(lambda a, b: dst[a:b], lambda a, b: src[a:b].float(), B)
    del dst
    # ... and back through split storage: fp16 values are their own hi part, the lo part is zero
    sp = ops.convert(src, ops.SPLIT)
    torch.cuda.synchronize()
    assert LG.equal_all_images(lambda a, b: sp[a:b].view(torch.float16).view(b - a, H, W, 2, C)[..., 0, :], lambda a, b: src[a:b], B)
    assert LG.equal_all_images(lambda a, b: sp[a:b].view(torch.int16).view(b - a, H, W, 2, C)[..., 1, :], lambda a, b: torch.zeros_like(src[a:b], dtype=torch.int16), B)


def test_nchw_to_nhwc_past_2g_elements(gpu):
    from resshift_amd import ops

    B, H, W, C = LG.ELEMENTWISE_SHAPE
    g = torch.Generator().manual_seed(LG.seed_of("nchw_to_nhwc"))
    src = LG.tile(torch.randn(P, C, H, W, generator=g).to(gpu), B).contiguous()
    assert src.numel() > LG.G31
    dst = ops.nchw_to_nhwc(src, prec=ops.F16)
    torch.cuda.synchronize()
    assert LG.equal_all_images(lambda a, b: dst[a:b], lambda a, b: src[a:b].permute(0, 2, 3, 1).half(), B)


def test_nhwc_to_nchw_past_2g_elements(gpu):
    from resshift_amd import ops

    B, H, W, C = LG.ELEMENTWISE_SHAPE
    g = torch.Generator().manual_seed(LG.seed_of("nhwc_to_nchw"))
    src = LG.tile(torch.randn(P, H, W, C, generator=g).to(gpu).half(), B).contiguous()
    assert src.numel() > LG.G31
    dst = ops.nhwc_to_nchw(src)
    torch.cuda.synchronize()
    assert LG.equal_all_images(lambda a, b: dst[a:b], lambda a, b: src[a:b].permute(0, 3, 1, 2).float(), B)


# ---------------------------------------------------------------- the engine's graph past 2^31 bytes
def test_realsr_encoder_at_batch_66_vs_oracle(gpu):
    """rs_vq_encode of the shipped realsr autoencoder at B = 66, 256 x 256, split storage: the first-level tensors are 66 x 32 MiB = 2.06 GiB
    (image 64 starts at byte 2^31).  z of EVERY image against the fp32 oracle of its base image (three distinct images along the batch)
    under the tolerance of test_autoencoder_vs_oracle; the nearest code of the engine's and of the oracle's latents may differ at no more
    than H.VQ_CAP = 0.1 % of an image's positions"""
    import helpers as H
    from oracle import resshift_oracle as oc
    from resshift_amd import ops
    from resshift_amd.engine import Engine
    from test_engine_gpu import TOL_NET

    B = 66
    _, ap, _ = H.realsr_params()
    per = int(ap["ddconfig"]["resolution"]) ** 2 * int(ap["ddconfig"]["ch"]) * 4
    assert (B - 2) * per == LG.G31 and LG.G31 < B * per < LG.LIMIT and LG.alias_visible(per)
    asd = H.synth.synthetic_state_dict(H.ae_param_spec(ap), H.SEED_W)
    eng = Engine(unet_params=None, ae_params=ap, device=gpu)
    eng.load_state_dicts(ae_sd=asd)
    eng.mark_weights_ready()
    base = torch.rand(P, 3, 256, 256, generator=torch.Generator().manual_seed(LG.seed_of("realsr encoder"))) * 2 - 1
    z = eng.vq_encode(LG.tile(base.to(gpu), B).contiguous(), prec=ops.SPLIT)
    torch.cuda.synchronize()
    ref = oc.vq_encode(asd, ap, base)
    e64 = asd["quantize.embedding.weight"].to(gpu).double()

    def nearest(t):
        zf = t.to(gpu).double().permute(0, 2, 3, 1).reshape(-1, e64.shape[1])
        return (torch.sum(zf ** 2, 1, keepdim=True) + torch.sum(e64 ** 2, 1) - 2 * zf @ e64.t()).argmin(1).view(t.shape[0], -1)

    want = nearest(ref)
    worst = differ = 0.0
    for b in range(B):
        worst = max(worst, H.rel_err(z[b:b + 1], ref[b % P:b % P + 1]))
        differ = max(differ, (nearest(z[b:b + 1]) != want[b % P:b % P + 1]).double().mean().item())
    print(f"\n[large] realsr encoder B = {B} split: first-level tensors {B * per / 2 ** 30:.3f} GiB, worst z error {worst:.3e} (tol {TOL_NET['split']:.0e}), "
          f"worst share of positions with another nearest code {differ:.2e} (cap {H.VQ_CAP:.0e})")
    del eng
    assert worst < TOL_NET["split"] and differ <= H.VQ_CAP, (worst, differ)


def test_realsr_decoder_folded_shortcut_past_2g(gpu):
    """The halo kernel's folded-shortcut source (IGemmParams::sx) past 2^31 bytes: no op-level entry passes sx, the engine does.  rs_vq_decode
    of the shipped realsr autoencoder at B = 33 in split storage: dec.up.0.block.0 is 256 -> 128 at 256 x 256 with a nin_shortcut that
    Graphs::skip_fold puts into conv2's launch, so sx is the block's input, 33 x 64 MiB = 2.06 GiB (conv1 reads the same tensor as x0).  The
    profiled pass must hold that launch - M = 33 * 256 * 256, N = 128, K = 9 * 128 + 256 on the split halo family - and EVERY image is
    compared with the fp32 oracle of its base latent under the tolerance of test_autoencoder_vs_oracle.  The latents are codebook rows plus
    noise far below the codebook's spacing, so the nearest code is not a matter of rounding: the indices must be the oracle's."""
    import helpers as H
    from oracle import resshift_oracle as oc
    from resshift_amd import ops
    from resshift_amd.engine import Engine
    from test_engine_gpu import TOL_NET

    B, h, w = 33, 64, 64
    _, ap, _ = H.realsr_params()
    dd = ap["ddconfig"]
    res, ch, mult = int(dd["resolution"]), int(dd["ch"]), [int(v) for v in dd["ch_mult"]]
    assert res == 4 * h and len(mult) == 3
    per = res * res * ch * mult[1] * 4           # bytes per image of up level 0's input in split storage
    assert LG.G31 < B * per < LG.LIMIT and LG.alias_visible(per)
    asd = H.synth.synthetic_state_dict(H.ae_param_spec(ap), H.SEED_W)
    eng = Engine(unet_params=None, ae_params=ap, device=gpu)
    eng.load_state_dicts(ae_sd=asd)
    eng.mark_weights_ready()
    g = torch.Generator().manual_seed(LG.seed_of("realsr decoder"))
    e = asd["quantize.embedding.weight"]
    codes = torch.randint(0, 256, (P, h, w), generator=g)   # (rows 0 .. 255: `spacing` below is their distance to the nearest OTHER row of the whole codebook)
    spacing = torch.cdist(e[:256].double(), e.double()).topk(2, largest=False).values[:, 1].min().item()
    base = e[codes].permute(0, 3, 1, 2).contiguous() + torch.randn(P, e.shape[1], h, w, generator=g) * (1e-3 * spacing)
    eng.profile_enable(True)
    try:
        d, idx = eng.vq_decode(LG.tile(base.to(gpu), B).contiguous(), prec=ops.SPLIT, return_indices=True)
        torch.cuda.synchronize()
        shapes, _ = eng.profile_shapes()
    finally:
        eng.profile_enable(False)
    folded = [s for s in shapes if s["part"] == "decoder" and (s["M"], s["N"], s["K"]) == (B * res * res, ch * mult[0], 9 * ch * mult[0] + ch * mult[1])]
    assert len(folded) == 1 and folded[0]["family"] == 1 and folded[0]["launches"] == 1, shapes   # (family 1: igemm4_kernel<*, true>, Engine.FAMILIES)
    ref, ref_idx = oc.vq_decode(asd, ap, base, return_indices=True)
    assert torch.equal(ref_idx.view(P, -1).long(), codes.view(P, -1)), "the oracle's nearest codes are not the rows the latents were made from"
    idx = idx.view(B, -1).cpu().long()
    worst = 0.0
    for b in range(B):
        assert torch.equal(idx[b], codes[b % P].view(-1)), f"image {b}: VQ indices differ from the oracle's"
        worst = max(worst, H.rel_err(d[b:b + 1], ref[b % P:b % P + 1]))
    print(f"\n[large] realsr decoder B = {B} split: folded-shortcut source {B * per / 2 ** 30:.3f} GiB, launch {folded[0]['M']} x {folded[0]['N']} x {folded[0]['K']}, "
          f"worst image error {worst:.3e} (tol {TOL_NET['split']:.0e})")
    del eng
    assert worst < TOL_NET["split"], worst

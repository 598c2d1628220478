"""Per-request seeds without a GPU: the float64 restatement of the noise definition (tests/_philox_ref.py) against published
known answers and against the moments of a standard normal; the C ABI additions (layout, exports, argument errors); the host logic of the
seeded ContinuousSampler / TilePool / sample_tiled / inference on recording fake engines; rs_sample_step_seeded's plumbing under the
test-hooks library with RS_FAKE_DEVICE=1."""
import ctypes
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import helpers as H
import _philox_ref as P
import _fakes
from _fakes import fake_launches, lib  # noqa: F401  (fixtures)
from oracle import cases
from resshift_amd import _lib, build
from resshift_amd.continuous import ContinuousSampler, request_seed
from resshift_amd.gaussian_diffusion import create_gaussian_diffusion
from resshift_amd.tilepool import TilePool, tile_windows

NO_GPU = {"HIP_VISIBLE_DEVICES": "-1"}


# ---------------------------------------------------------------------------------------------------------------- the definition
KNOWN_WORDS = [   # counter, key, words: the first and third are Random123's published Philox4x32-10 vectors
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,words", KNOWN_WORDS)
def test_restatement_reproduces_the_known_philox_words(counter, key, words):
    assert tuple(int(w[0]) for w in P.philox4x32_10(counter, key)) == words


def test_restatement_reproduces_the_known_normals():
    a = P.normals(10000, 3, 7, 6)
    np.testing.assert_allclose(a, [-0.268851116, -1.502480008, -0.086357182, -0.695469991, 0.886042956, 0.990155076], rtol=0, atol=1e-9)
    b = P.normals(2 ** 63 + 12345, 0xffffffff, 15, 5)   # a count that is no multiple of 4 drops the surplus
    np.testing.assert_allclose(b, [-1.170016172, 1.277732689, -1.058624807, -0.027614715, -0.066186654], rtol=0, atol=1e-9)
    assert b.shape == (5,) and np.array_equal(P.normals(2 ** 63 + 12345, 0xffffffff, 15, 8)[:5], b)
    assert np.abs(P.normals(1, 0, 0, 1 << 16)).max() <= np.sqrt(48 * np.log(2))


def test_restatement_moments_and_independence_of_streams_seeds_and_draws():
    """2^22 normals of (seed 10000, stream 0, draw 0), (10000, 1, 0), (10001, 0, 0), (10000, 0, 1): mean, variance, fourth moment and the
    correlation of the first with the other three, each within five standard errors of a standard normal's"""
    N = 1 << 22
    sets = [P.normals(*k, N) for k in ((10000, 0, 0), (10000, 1, 0), (10001, 0, 0), (10000, 0, 1))]
    for i, a in enumerate(sets):
        mean, var, m4 = a.mean(), a.var(), np.mean(a ** 4)
        print(f"set {i}: mean {mean * np.sqrt(N):+.2f} se, var {(var - 1) / np.sqrt(2 / N):+.2f} se, m4 {(m4 - 3) / np.sqrt(96 / N):+.2f} se")
        assert abs(mean) < 5 / np.sqrt(N)
        assert abs(var - 1) < 5 * np.sqrt(2 / N)
        assert abs(m4 - 3) < 5 * np.sqrt(96 / N)
    for i in (1, 2, 3):
        c = np.mean(sets[0] * sets[i])
        print(f"E[set0 set{i}] = {c * np.sqrt(N):+.2f} se")
        assert abs(c) < 5 / np.sqrt(N)


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_noise_key_layout_and_exports(lib):
    assert ctypes.sizeof(_lib.NoiseKey) == 16
    assert [f[0] for f in _lib.NoiseKey._fields_] == ["seed", "stream", "reserved"]
    assert (_lib.NoiseKey.seed.offset, _lib.NoiseKey.stream.offset, _lib.NoiseKey.reserved.offset) == (0, 8, 12)
    for sym in ("rs_noise_fill", "rs_sample_seeded", "rs_sample_begin_seeded", "rs_sample_step_seeded"):
        assert sym in _lib.SIGNATURES and hasattr(lib, sym), sym
    k = _lib.noise_keys([(2 ** 64 + 5, 7), 9, (-1, 0)])
    assert [(int(q.seed), int(q.stream), int(q.reserved)) for q in k] == [(5, 7, 0), (9, 0, 0), (2 ** 64 - 1, 0, 0)]
    with pytest.raises(ValueError, match="32 bits"):
        _lib.noise_keys([(1, 2 ** 32)])
    # the existing structs keep their layout (rs_sample_args / rs_step_args are passed beside the keys, unchanged)
    assert ctypes.sizeof(_lib.StepArgs) == 8 * 7 + 4 * 2 + 8


def test_noise_fill_argument_errors_fire_without_a_device(lib):
    keys, draw = _lib.noise_keys([(1, 0), (2, 0)]), (ctypes.c_int * 2)(0, 1)
    out = 4096   # never dereferenced: every case below is rejected before anything is launched
    cases_ = {
        "B must be": lambda: lib.rs_noise_fill(keys, draw, out, 16, 0, None),
        "RS_MAX_ROWS": lambda: lib.rs_noise_fill(keys, draw, out, 16, _lib.RS_MAX_ROWS + 1, None),
        "null keys": lambda: lib.rs_noise_fill(None, draw, out, 16, 2, None),
        "null draw": lambda: lib.rs_noise_fill(keys, None, out, 16, 2, None),
        "output": lambda: lib.rs_noise_fill(keys, draw, None, 16, 2, None),
        "per_image_count": lambda: lib.rs_noise_fill(keys, draw, out, 0, 2, None),
        "negative draw": lambda: lib.rs_noise_fill(keys, (ctypes.c_int * 2)(0, -1), out, 16, 2, None),
    }
    for text, fn in cases_.items():
        assert fn() == -2, text
        assert text in _lib.last_error(), (text, _lib.last_error())
    keys[1].reserved = 3
    assert lib.rs_noise_fill(keys, draw, out, 16, 2, None) == -2 and "reserved" in _lib.last_error()
    sa = _lib.SampleArgs()
    sa.B = 2
    for fn in (lambda k: lib.rs_sample_seeded(4096, ctypes.byref(sa), k), lambda k: lib.rs_sample_begin_seeded(4096, ctypes.byref(sa), 4096, k)):
        assert fn(None) == -2 and "null keys" in _lib.last_error()
        assert fn(keys) == -2 and "reserved" in _lib.last_error()
    sa.B = 0
    assert lib.rs_sample_seeded(4096, ctypes.byref(sa), keys) == -2 and "B must be" in _lib.last_error()


# ---------------------------------------------------------------------------------------------------------------- schedulers (fake engine)
class FakeEngine:
    """tests/test_continuous_cpu.py's recording engine with the keys= parameter of the real one: x[:, 0, 0, 0] carries the image's id (its LR
    fill value), x[:, 1, 0, 0] counts the steps; every call is recorded with the keys it got.  A noise tensor is an error."""

    def __init__(self):
        self.calls = []

    def latent_shape(self, B, h, w, sf):
        return (B, 3, h * sf // 4, w * sf // 4)

    def film_prewarm(self, timesteps):
        pass

    def sample_begin(self, y, noise, tables, sf, scale_factor, prec_encode=None, out=None, keys=None):
        assert noise is None and keys is not None and len(keys) == y.shape[0] and out is not None and out.is_contiguous()
        out.zero_()
        out[:, 0, 0, 0] = y[:, 0, 0, 0]
        self.calls.append(("begin", torch.round(y[:, 0, 0, 0] * 1000).long().tolist(), list(keys)))
        return out

    def sample_step(self, x, y, t, noise, tables, sf, mask=None, prec=None, pred_xstart=None, keys=None):
        assert noise is None and keys is not None and len(keys) == len(t) == x.shape[0] == y.shape[0]
        assert torch.equal(x[:, 0, 0, 0], y[:, 0, 0, 0])
        x[:, 1, 0, 0] += 1
        self.calls.append(("step", torch.round(x[:, 0, 0, 0] * 1000).long().tolist(), list(t), list(keys)))
        return x

    def sample_end(self, x0, h, w, sf, scale_factor, prec_decode=None, return_aux=False):
        self.calls.append(("end", torch.round(x0[:, 0, 0, 0] * 1000).long().tolist()))
        return x0[:, 0, 0, 0].view(-1, 1, 1, 1).expand(-1, 3, h * sf, w * sf).contiguous() * 1.0


def fake_sampler(**kw):
    return _fakes.fake_sampler(engine=FakeEngine(), **kw)


def lq_of(code, h=16, w=16):
    return torch.full((1, 3, h, w), code / 1000.0)


def test_seeded_scheduler_passes_keys_keeps_them_with_their_slots_and_stores_no_draws():
    """staggered arrivals as in test_scheduler_admits_steps_retires_and_compacts: every call carries, slot by slot, the key of the image in
    that slot - through admission, mixed steps, retirement and compaction - and no noise tensor exists anywhere"""
    s = fake_sampler()
    cs = ContinuousSampler(s, max_batch=4, seeded=True)
    arrivals = {0: 2, 1: 1, 3: 2, 5: 1}
    key_of, got, k = {}, {}, 0
    while k < 6 or cs.pending():
        for _ in range(arrivals.get(k, 0)):
            i = len(key_of)
            if i % 2:
                rid, = cs.submit(lq_of(i), seed=500 + i, stream=i)
                key_of[rid] = (500 + i, i)
            else:   # the default: derived from the sampler's seed and the request id
                rid, = cs.submit(lq_of(i))
                key_of[rid] = (request_seed(77, rid), 0)
            assert rid == i
        got.update(cs.step())
        assert cs._N is None
        k += 1
    assert sorted(got) == list(range(6)) and cs._N is None and cs._keys == []
    steps_seen = {i: [] for i in range(6)}
    for c in s.engine.calls:
        if c[0] == "begin":
            assert c[2] == [key_of[i] for i in c[1]]
        elif c[0] == "step":
            assert c[3] == [key_of[i] for i in c[1]], c
            for i, t in zip(c[1], c[2]):
                steps_seen[i].append(t)
    assert all(v == list(range(cs.steps - 1, -1, -1)) for v in steps_seen.values())
    assert any(len(set(c[2])) > 1 for c in s.engine.calls if c[0] == "step")          # mixed steps happened
    slots = [c[1] for c in s.engine.calls if c[0] == "step"]
    assert any(a[0] != b[0] for a, b in zip(slots, slots[1:]) if a and b)             # ... and a compaction moved images between slots
    assert request_seed(77, 3) == 77 * 2 ** 32 + 3 and request_seed(2 ** 40, 1) == (2 ** 72 + 1) % 2 ** 64


def test_seeded_mode_rejects_tensors_and_default_mode_rejects_seeds():
    z = torch.zeros(1, 3, 16, 16)
    cs = ContinuousSampler(fake_sampler(), seeded=True)
    with pytest.raises(ValueError, match="not accepted"):
        cs.submit(lq_of(0), noise=z)
    with pytest.raises(ValueError, match="not accepted"):
        cs.submit(lq_of(0), step_noises=[z] * cs.steps)
    with pytest.raises(NotImplementedError, match="noise_repeat"):
        cs.submit(lq_of(0), noise_repeat=True)
    with pytest.raises(ValueError, match="2 images but 1 seeds"):
        cs.submit(torch.cat([lq_of(0), lq_of(1)]), seed=[4])
    assert cs.submit(torch.cat([lq_of(0), lq_of(1)]), seed=[4, 5]) == [0, 1]
    with pytest.raises(ValueError, match="seeded=True"):
        ContinuousSampler(SimpleNamespace(**{**fake_sampler().__dict__, "engine": _TensorEngine()})).submit(lq_of(0), seed=3)
    tp = TilePool(fake_sampler(), seeded=True)
    with pytest.raises(ValueError, match="not accepted"):
        tp.submit(lq_of(0)[0], tile_noises=[(z, [z] * tp.steps)])
    with pytest.raises(ValueError, match="seeded=True"):
        TilePool(SimpleNamespace(**{**fake_sampler().__dict__, "engine": _TensorEngine()})).submit(lq_of(0)[0], seed=3)


class _TensorEngine(FakeEngine):
    """the engine of a default-mode pool is never reached by the rejected calls above"""


def test_tile_j_of_an_image_gets_stream_j(fake_launches):
    """two images (six tiles and three) in a seeded pool of 4: every row of every engine call carries (its image's seed, its tile index)"""
    s = fake_sampler()
    tp = TilePool(s, max_batch=4, seeded=True)
    sizes, seeds = [(40, 28), (12, 40)], [901, None]
    want = {}
    for i, ((h, w), sd) in enumerate(zip(sizes, seeds)):
        img = torch.zeros(3, h, w)
        wins = tile_windows(h, w, 16, 12)
        for j, (h0, w0, _, _) in enumerate(wins):   # a tile's code sits on its top-left pixel (tile origins are distinct)
            img[:, h0, w0] = (i * 16 + j + 1) / 1000.0
            want[i * 16 + j + 1] = (sd if sd is not None else request_seed(77, i), j)
        assert tp.submit(img, seed=sd) == i
    assert len(want) == 9
    out = tp.drain()
    assert sorted(out) == [0, 1]
    seen = set()
    for c in s.engine.calls:
        if c[0] in ("begin", "step"):
            assert c[-1] == [want[code] for code in c[1]], c
            seen.update(c[1])
    assert seen == set(want)
    assert all(cl.cs._N is None for cl in tp._classes.values())


def test_sample_tiled_gives_tile_j_stream_j_for_any_chop_bs():
    from resshift_amd.sampler import ResShiftSampler

    for chop_bs in (1, 2, 4):
        s = ResShiftSampler.__new__(ResShiftSampler)
        s.chop_size, s.chop_stride, s.chop_bs, s.sf = 16, 12, chop_bs, 4
        calls = []

        def sample_func(pch, noise_repeat=False, mask=False, noise=None, step_noises=None, seeds=None, _calls=calls):
            assert noise is None and step_noises is None and len(seeds) == pch.shape[0]
            _calls.append((torch.round(pch[:, 0, 0, 0]).long().tolist(), list(seeds)))
            return torch.zeros(pch.shape[0], 3, pch.shape[2] * 4, pch.shape[3] * 4)

        s.sample_func = sample_func

        class Splitter:   # TileSplitter's batch layout (tile kk of the call, image b -> row kk * B0 + b) without its device kernels
            def __init__(self, im, pch_size, stride, sf, extra_bs):
                self.im, self.bs = im, extra_bs
                self.starts = [(h0, w0) for h0, w0, _, _ in tile_windows(im.shape[2], im.shape[3], pch_size, stride)]

            def __iter__(self):
                for k in range(0, len(self.starts), self.bs):
                    cur = self.starts[k:k + self.bs]
                    yield torch.cat([self.im[:, :, h0:h0 + 16, w0:w0 + 16] for h0, w0 in cur]), [[0, 0, 0, 0]] * len(cur)

            def update(self, out, infos):
                pass

            def gather(self):
                return None

        import resshift_amd.tiling as tiling
        old, tiling.TileSplitter = tiling.TileSplitter, Splitter
        try:
            im = torch.zeros(2, 3, 40, 28)
            for j, (h0, w0, _, _) in enumerate(tile_windows(40, 28, 16, 12)):
                im[0, :, h0, w0], im[1, :, h0, w0] = j, 100 + j          # code: image * 100 + tile index
            s.sample_tiled(im, seed=[11, 22])
            small = s.sample_tiled(torch.zeros(2, 3, 16, 12), seed=[11, 22])  # untiled: tile 0
        finally:
            tiling.TileSplitter = old
        flat = [(c, k) for codes, keys in calls[:-1] for c, k in zip(codes, keys)]
        assert sorted(flat) == sorted([(j, (11, j)) for j in range(6)] + [(100 + j, (22, j)) for j in range(6)]), (chop_bs, flat)
        assert calls[-1][1] == [(11, 0), (22, 0)] and small is not None
        with pytest.raises(ValueError, match="excludes"):
            s.sample_tiled(im, seed=3, noise_repeat=True)


@pytest.mark.parametrize("pool", [False, True])
def test_inference_seeded_gives_a_file_the_same_seed_for_any_world_size(tmp_path, monkeypatch, pool):
    """seven files, bs 4 and 6, world sizes 1, 2 and 3: the seed of a file is image_seed(its position in the sorted listing), whichever
    rank reads it and with or without the pool"""
    from PIL import Image

    import resshift_amd.tilepool as tilepool
    from resshift_amd.sampler import ResShiftSampler

    src = tmp_path / "in"
    src.mkdir()
    names = [f"im{i:02d}" for i in range(7)]
    for i, n in enumerate(names):
        Image.fromarray(np.full((8, 8, 3), i, dtype=np.uint8)).save(src / f"{n}.png")
    seen = {}

    def record(code, seed):
        seen.setdefault(code, set()).add(int(seed))

    class Pool(_fakes.InstantPool):
        def finished(self, lq, seed):
            assert self.seeded
            record(int(lq[0, 0, 0, 0]), seed)
            return torch.zeros(3, 32, 32)

    monkeypatch.setattr(tilepool, "TilePool", Pool)
    eng = SimpleNamespace(u8_to_input=lambda t: t.permute(0, 3, 1, 2).float(),
                          output_to_u8=lambda sr, lq=None, mask=None: torch.zeros(sr.shape[0], 32, 32, 3, dtype=torch.uint8))
    runs = 0
    for world in (1, 2, 3):
        for bs in (4, 6):
            for rank in range(world):
                s = ResShiftSampler.__new__(ResShiftSampler)
                s.seed, s.rank, s.num_gpus, s.device, s.engine, s.chop_size = 4242, rank, world, torch.device("cpu"), eng, 128

                def sample_tiled(lq, mask=None, noise_repeat=False, tile_noises=None, seed=None):
                    assert len(seed) == lq.shape[0]
                    for j in range(lq.shape[0]):
                        record(int(lq[j, 0, 0, 0]), seed[j])
                    return torch.zeros(lq.shape[0], 3, 32, 32)

                s.sample_tiled = sample_tiled
                s.inference(src, tmp_path / f"out_{world}_{bs}", bs=bs, pool=pool, seeded=True)
                runs += 1
    assert runs == 12
    want = {i: {request_seed(4242, i)} for i in range(7)}
    assert seen == want, seen
    with pytest.raises(ValueError, match="noise_repeat"):
        s.inference(src, tmp_path / "x", seeded=True, noise_repeat=True)


# ---------------------------------------------------------------------------------------------------------------- plumbing
def test_seeded_step_dry_and_real_pass_agree_and_cost_the_launches_of_the_tensor_step():
    """rs_sample_step_seeded at realsr B = 32 (split): the dry and the real pass agree for a uniform and for a mixed step, and each costs
    exactly the launches of rs_sample_step; key errors fire with clear messages and rs_sample_step keeps its own"""
    env = dict(os.environ, RS_FAKE_DEVICE="1", RESSHIFT_HIP_LIB=build.build_testhooks(), **NO_GPU)
    r = subprocess.run([sys.executable, os.path.join(H.ROOT, "tests", "_fake_device_step_seeded.py"), "32", "2"], env=env, capture_output=True,
                       text=True, timeout=600)
    fd = re.findall(r"dry: tickets (\d+) pool (\d+) prod (\d+) gn (\d+) \| real: tickets (\d+) pool (\d+) prod (\d+) gn (\d+) launches (\d+)", r.stderr)
    assert len(fd) == 4, (r.stdout[-800:], r.stderr[-1500:])
    for m in fd:
        v = [int(x) for x in m]
        assert v[:4] == v[4:8] and v[0] > 0, v
    assert "never attached" not in r.stderr, r.stderr[-500:]
    calls = dict((m[0], int(m[1])) for m in re.findall(r"CALL (\w+) rc -?\d+ launches (\d+)", r.stdout))
    assert calls["seeded_uniform"] == calls["tensor_uniform"] > 0, calls
    assert calls["seeded_mixed"] == calls["tensor_mixed"] == calls["tensor_uniform"] + 1, calls
    errs = {m[0]: (int(m[1]), m[2]) for m in re.findall(r"ERR (\w+) rc (-?\d+) (.*)", r.stdout)}
    assert errs["null_keys"] == (-2, "rs_sample_step_seeded: null keys"), errs
    assert errs["reserved"][0] == -2 and "keys[31].reserved" in errs["reserved"][1], errs
    assert errs["b_zero"][0] == -2 and "B must be" in errs["b_zero"][1], errs
    assert "RS_MAX_ROWS" in errs["b_bound_mixed"][1], errs
    assert "noise is NULL" in errs["tensor_null_noise"][1], errs

"""Feathered tile blending without a GPU: the properties of the float64 restatement (tests/_feather_ref.py), the argument
errors of rs_tile_accumulate_weighted / rs_tile_scatter_weighted - found before anything is launched - and the host plumbing from
`tile_blend=` down to the weighted calls, on recording fakes in the manner of tests/test_tilepool_cpu.py."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers as H  # noqa: F401  (puts the repository root on sys.path)
import _feather_ref as R
from _fakes import _OnDevice, fake_sampler, lib  # noqa: F401  (fixtures)
from resshift_amd import _lib, tiling
from resshift_amd.tilepool import TilePool, tile_windows


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("n,Rr", [(64, 16), (48, 16), (64, 0), (8, 3), (5, 3), (1, 4), (21, 12), (64, 64)])
def test_weights_are_symmetric_and_lie_in_0_1(n, Rr):
    w = R.w1(n, Rr)
    assert w.shape == (n,) and w.dtype == np.float64
    assert np.array_equal(w, w[::-1])
    assert np.all(w > 0) and np.all(w <= 1)
    if Rr == 0:
        assert np.all(w == 1)
    else:
        assert w[0] == 0.5 / Rr or n == 1 and w[0] == min(1.0, 0.5 / Rr)
        assert np.all(np.diff(w[:(n + 1) // 2]) >= 0)          # rises towards the middle
        if n >= 2 * Rr:
            assert np.all(w[Rr:n - Rr] == 1)                    # a plateau of full weight between the two ramps
        else:
            assert w.max() == min(1.0, ((n - 1) // 2 + 0.5) / Rr)   # a cropped tile ramps up to less than one
    w2 = R.weight(n, 7, Rr, 2)
    assert w2.shape == (n, 7) and np.array_equal(w2, np.outer(w, R.w1(7, 2)))


def test_seam_property_two_constant_tiles():
    """chop 16 / stride 12 / sf 4: tiles of 64 HR pixels, overlap R = 16.  Tile A = +1 at column 0, tile B = -1 at column 48."""
    chop, stride, sf = 16, 12, 4
    Rr, n = R.ramp(chop, stride, sf), chop * sf
    assert (Rr, n) == (16, 64)
    x0 = stride * sf
    tiles = [(np.full((n, n), 1.0), 0, 0), (np.full((n, n), -1.0), 0, x0)]
    out = R.blend((n, x0 + n), tiles, Rr, Rr)
    p = np.arange(Rr)
    assert np.all(out[:, :x0] == 1) and np.all(out[:, n:] == -1)                   # one tile: its weight cancels
    np.testing.assert_allclose(out[:, x0:n], np.broadcast_to((Rr - 1 - 2 * p) / Rr, (n, Rr)), rtol=0, atol=1e-15)
    assert np.abs(np.diff(out, axis=1)).max() == pytest.approx(2 / Rr, abs=1e-15)
    assert np.abs(np.diff(out, axis=0)).max() == 0
    uni = R.blend((n, x0 + n), tiles, 0, 0)
    assert np.all(uni[:, x0:n] == 0) and np.abs(np.diff(uni, axis=1)).max() == 1   # the uniform average steps by one at both edges


# ---------------------------------------------------------------------------------------------------------------- C ABI
PTR = 0x1000   # never dereferenced: every call below is refused before anything is launched


def _descs(*rows):
    arr = (_lib.TileDesc * max(1, len(rows)))()
    for d, r in zip(arr, rows):
        d.src, d.acc, d.count, d.H, d.W, d.h0, d.w0, d.th, d.tw = r
    return arr


SCATTER_ERRORS = {
    "Rh_negative": (dict(Rh=-1), "must not be negative"),
    "Rw_negative": (dict(Rw=-16), "must not be negative"),
    "n_zero": (dict(n=0), "outside 1 .. RS_MAX_ROWS"),
    "n_large": (dict(n=_lib.RS_MAX_ROWS + 1), "outside 1 .. RS_MAX_ROWS"),
    "null_desc": (dict(desc=None), "null descriptor array"),
    "channels": (dict(C=0), "must be positive"),
    "sf": (dict(sf=0), "must be positive"),
    "null_tiles": (dict(tiles=None), "null tensor (tiles)"),
    "null_acc": (dict(rows=[(None, None, PTR, 40, 28, 0, 0, 16, 16)]), "desc.acc / desc.count"),
    "null_count": (dict(rows=[(None, PTR, None, 40, 28, 0, 0, 16, 16)]), "desc.acc / desc.count"),
    "window": (dict(rows=[(None, PTR, PTR, 40, 28, 28, 12, 16, 16)]), "leaves its plane"),
    "tile_tensor_small": (dict(rows=[(None, PTR, PTR, 40, 28, 0, 0, 17, 16)]), "th*sf > Hp_out or tw*sf > Wp_out"),
    "canvas_count": (dict(rows=[(None, PTR, PTR, 40, 28, 0, 0, 16, 16), (None, PTR, PTR + 64, 40, 28, 0, 12, 16, 16)]), "disagree"),
    "canvas_size": (dict(rows=[(None, PTR, PTR, 40, 28, 0, 0, 16, 16), (None, PTR, PTR, 40, 32, 0, 12, 16, 16)]), "disagree"),
}


@pytest.mark.parametrize("name", sorted(SCATTER_ERRORS))
def test_tile_scatter_weighted_argument_errors(lib, name):
    """a negative ramp, and everything rs_tile_scatter rejects (tests/test_tilepool_cpu.py's cases)"""
    kw, text = SCATTER_ERRORS[name]
    a = dict(C=3, sf=4, tiles=PTR, Rh=16, Rw=16, rows=[(None, PTR, PTR, 40, 28, 24, 12, 16, 16)])
    a.update({k: v for k, v in kw.items() if k not in ("desc", "n")})
    n = kw.get("n", len(a["rows"]))
    desc = None if "desc" in kw else _descs(*(a["rows"] * (n if "n" in kw else 1))[:_lib.RS_MAX_ROWS])
    rc = lib.rs_tile_scatter_weighted(desc, n, a["C"], a["sf"], a["tiles"], 64, 64, a["Rh"], a["Rw"], None)
    assert rc == -2 and text in _lib.last_error() and _lib.last_error().startswith("rs_tile_scatter_weighted: "), (rc, _lib.last_error())


ACCUMULATE_ERRORS = {
    "Rh_negative": (dict(Rh=-1), "must not be negative"),
    "Rw_negative": (dict(Rw=-1), "must not be negative"),
    "null_acc": (dict(acc=None), "null tensor"),
    "null_count": (dict(count=None), "null tensor"),
    "null_tile": (dict(tile=None), "null tensor"),
    "window_right": (dict(w0=49), "leaves its canvas"),
    "window_bottom": (dict(h0=97), "leaves its canvas"),
    "window_negative": (dict(h0=-1), "leaves its canvas"),
    "window_empty": (dict(tw=0), "leaves its canvas"),
    "batch": (dict(B=0), "leaves its canvas"),
}


@pytest.mark.parametrize("name", sorted(ACCUMULATE_ERRORS))
def test_tile_accumulate_weighted_argument_errors(lib, name):
    kw, text = ACCUMULATE_ERRORS[name]
    a = dict(acc=PTR, count=PTR, tile=PTR, B=1, C=3, H=160, W=112, h0=96, w0=48, th=64, tw=64, Rh=16, Rw=16)
    a.update(kw)
    rc = lib.rs_tile_accumulate_weighted(a["acc"], a["count"], a["tile"], a["B"], a["C"], a["H"], a["W"], a["h0"], a["w0"], a["th"], a["tw"],
                                         a["Rh"], a["Rw"], None)
    assert rc == -2 and text in _lib.last_error() and _lib.last_error().startswith("rs_tile_accumulate_weighted: "), (rc, _lib.last_error())


def test_the_new_symbols_are_declared_and_the_descriptor_keeps_its_layout(lib):
    import ctypes

    for name, n_args in (("rs_tile_accumulate_weighted", 14), ("rs_tile_scatter_weighted", 10)):
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == n_args
    assert len(_lib.SIGNATURES["rs_tile_scatter_weighted"][1]) == len(_lib.SIGNATURES["rs_tile_scatter"][1]) + 2
    assert ctypes.sizeof(_lib.TileDesc) == 48   # the ramp widths travel as kernel arguments, not in the descriptor


# ---------------------------------------------------------------------------------------------------------------- host plumbing
CODE = 1e-3   # a tile's code travels as code * CODE, so that it survives the clamp to [-1, 1]


@pytest.fixture
def fake_launches(monkeypatch):
    """torch restatements of the pool's launches (the weights are the restatement's); every scatter call is recorded as it was made"""
    log = []

    def gather(tiles, out_lq, out_mask=None):
        Hp, Wp = out_lq.shape[-2:]
        for k, (src, h0, w0, th, tw) in enumerate(tiles):
            out_lq[k] = F.pad(src[None, :3, h0:h0 + th, w0:w0 + tw], (0, Wp - tw, 0, Hp - th), mode="reflect")[0]

    def scatter(*args, **kwargs):
        log.append((len(args), dict(kwargs)))
        tiles, batch, sf = args
        Rh, Rw = kwargs.get("ramp") or (0, 0)
        for k, (acc, cnt, Hh, W, h0, w0, th, tw) in enumerate(tiles):
            w = torch.from_numpy(R.weight(th * sf, tw * sf, Rh, Rw)).float()
            acc[:, h0 * sf:(h0 + th) * sf, w0 * sf:(w0 + tw) * sf] += w * batch[k, :, :th * sf, :tw * sf]
            cnt[h0 * sf:(h0 + th) * sf, w0 * sf:(w0 + tw) * sf] += w

    monkeypatch.setattr(_lib, "tile_gather", gather)
    monkeypatch.setattr(_lib, "tile_scatter", scatter)
    monkeypatch.setattr(_lib, "tile_finalize", lambda acc, count: acc.div_(count))
    return log


def _coded(i, Hh, W):
    lq = torch.zeros(3, Hh, W)
    wins = tile_windows(Hh, W, 16, 12)
    for k, (h0, w0, _, _) in enumerate(wins):
        lq[0, h0, w0] = (16 * i + k + 1) * CODE
    return lq, wins


def _expected(i, Hh, W, wins, sf, Rr):
    tiles = [(np.full((3, th * sf, tw * sf), np.float32((16 * i + k + 1) * CODE), dtype=np.float64), h0 * sf, w0 * sf)
             for k, (h0, w0, th, tw) in enumerate(wins)]
    return R.blend((3, Hh * sf, W * sf), tiles, Rr, Rr)


@pytest.mark.parametrize("seeded", [False, True])
@pytest.mark.parametrize("blend", ["uniform", "feather", None])
def test_tile_pool_reads_the_blend_from_its_sampler(fake_launches, blend, seeded):
    """feather: every retirement is ONE tile_scatter call with ramp = (chop_size - chop_stride) * sf for both axes, and the images are the
    restatement's; uniform - named, or a sampler without the attribute - issues exactly the calls it always has: three arguments"""
    s = fake_sampler(**({"tile_blend": blend} if blend else {}))
    tp = TilePool(s, max_batch=4, seeded=seeded)
    sizes = [(40, 28), (12, 40), (13, 10)]      # six tiles, three cropped ones, one whole image
    wins = {}
    for i, (Hh, W) in enumerate(sizes):
        lq, wins[i] = _coded(i, Hh, W)
        assert tp.submit(lq) == i
    out = tp.drain()
    Rr = (16 - 12) * tp.sf
    assert Rr == 16 and sorted(out) == [0, 1, 2] and fake_launches
    if blend == "feather":
        assert (tp.blend, tp.ramp) == ("feather", (Rr, Rr))
        assert all(call == (3, {"ramp": (Rr, Rr)}) for call in fake_launches), fake_launches
    else:
        assert (tp.blend, tp.ramp) == ("uniform", None)
        assert all(call == (3, {}) for call in fake_launches), fake_launches
    for i, (Hh, W) in enumerate(sizes):
        want = _expected(i, Hh, W, wins[i], tp.sf, Rr if blend == "feather" else 0)
        np.testing.assert_allclose(out[i].numpy(), want, rtol=0, atol=1e-7)   # values below 0.05, a handful of fp32 roundings each
    # constant tiles of different values: the two blends differ wherever tiles overlap (and only the uniform one steps)
    assert blend != "feather" or not np.allclose(out[0].numpy(), _expected(0, 40, 28, wins[0], tp.sf, 0), rtol=0, atol=1e-6)


def test_unknown_blend_is_rejected():
    from resshift_amd.sampler import ResShiftSampler

    with pytest.raises(ValueError, match="unknown tile blend 'gauss'"):
        TilePool(fake_sampler(tile_blend="gauss"))
    with pytest.raises(ValueError, match="unknown tile blend"):
        ResShiftSampler({}, tile_blend="gauss")          # validated like `precision`: before anything is built
    with pytest.raises(ValueError, match="unknown precision"):
        ResShiftSampler({}, precision="fp8", tile_blend="feather")
    with pytest.raises(ValueError, match="unknown tile blend"):
        tiling.check_blend(None)
    assert tiling.BLENDS == ("uniform", "feather") and tiling.feather_ramp(16, 12, 4) == (16, 16) and tiling.feather_ramp(8, 8, 2) == (0, 0)


@pytest.mark.parametrize("seed", [None, 5])
@pytest.mark.parametrize("chop_bs", [1, 4])
@pytest.mark.parametrize("blend", ["uniform", "feather"])
def test_sample_tiled_honours_the_blend(monkeypatch, blend, chop_bs, seed):
    """sample_tiled -> TileSplitter -> the engine's calls, recorded: feather issues one rs_tile_accumulate_weighted per tile with the HR
    origin and R = (chop_size - chop_stride) * sf; uniform issues exactly rs_tile_accumulate's twelve arguments per tile; an untiled
    image reaches neither"""
    from resshift_amd.sampler import ResShiftSampler

    calls = []
    fake_lib = SimpleNamespace(rs_tile_accumulate=lambda *a: calls.append(("uniform", a)) or 0,
                               rs_tile_finalize=lambda *a: calls.append(("finalize", a)) or 0)
    monkeypatch.setattr(_lib, "load", lambda: fake_lib)
    monkeypatch.setattr(_lib, "window_copy", lambda x, h0, w0, ho, wo, out=None: out.copy_(x[..., h0:h0 + ho, w0:w0 + wo]))
    monkeypatch.setattr(_lib, "tile_accumulate_weighted",
                        lambda acc, count, tile, h0, w0, ramp: calls.append(("feather", (tuple(acc.shape), tuple(count.shape), tuple(tile.shape), h0, w0, ramp))))
    s = ResShiftSampler.__new__(ResShiftSampler)
    s.chop_size, s.chop_stride, s.chop_bs, s.sf, s.tile_blend = 16, 12, chop_bs, 4, blend
    seen_seeds = []

    def sample_func(pch, noise_repeat=False, mask=None, noise=None, step_noises=None, seeds=None):
        seen_seeds.append(seeds)
        return torch.zeros(pch.shape[0], 3, pch.shape[2] * 4, pch.shape[3] * 4)

    s.sample_func = sample_func
    im = torch.zeros(1, 3, 40, 28).as_subclass(_OnDevice)
    out = s.sample_tiled(im, seed=seed)
    wins = tile_windows(40, 28, 16, 12)
    assert tuple(out.shape) == (1, 3, 160, 112) and len(wins) == 6
    assert all((sd is None) == (seed is None) for sd in seen_seeds) and len(seen_seeds) == -(-6 // chop_bs)
    kinds = [c[0] for c in calls]
    assert kinds == [blend] * 6 + ["finalize"]
    for (kind, a), (h0, w0, th, tw) in zip(calls, wins):
        if blend == "feather":
            assert a == ((1, 3, 160, 112), (160, 112), (1, 3, 64, 64), h0 * 4, w0 * 4, (16, 16))
        else:
            assert len(a) == 12 and a[3:11] == (1, 3, 160, 112, h0 * 4, w0 * 4, th * 4, tw * 4)
    del calls[:]
    s.sample_tiled(torch.zeros(1, 3, 16, 12).as_subclass(_OnDevice), seed=seed)    # one tile: straight to sample_func
    assert calls == []

"""Feathered tile blending on the GPU (tiny shapes, the file prints its wall time).  The reference is the float64
restatement of the definition, tests/_feather_ref.py.

  * rs_tile_scatter_weighted against rs_tile_accumulate_weighted tile by tile, and with R = 0 against rs_tile_scatter, bit for bit;
  * scatter + finalize against the restatement, and the seam property (no step larger than 2/R between neighbouring pixels);
  * end to end: sample_tiled(seed=) under tile_blend="feather" against the restatement fed with the tiles' own outputs, and the tile
    pool against sample_tiled, bit for bit.

The shapes are those of tests/test_tilepool_gpu.py::test_tile_scatter_equals_accumulate_tile_by_tile: sf 4, canvases 40 x 28 and 12 x 40 at
chop 16 / stride 12 (four-fold overlap, R = 16, cropped tiles of 48 rows, the 16-byte path); sf 1, canvases 13 x 21 and 8 x 19 at chop 8 /
stride 5 (R = 3: weights that are no dyadic fractions, the scalar path).  In neither is a tile side shorter than two ramps, so a third
layout adds that: sf 4, canvases 3 x 28 and 40 x 5 at chop 16 / stride 12 - tiles of 12 rows resp. 20 columns under R = 16, whose two
ramps meet below full weight.  Tiles of the two canvases are interleaved and two launches land on the same canvases.
"""
import time

import numpy as np
import pytest
import torch

import helpers as H
import _feather_ref as R
from oracle import make_golden_tiled as mt

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL = 2e-6   # absolute, on inputs in [-1, 1]: each term's error is relative to w |v| <= w and the denominator is the sum of the w, so a
#              dozen fp32 roundings give <= 12 * 2^-24 = 7e-7; an index or ramp mistake is O(1/R) or larger
_T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    yield
    print(f"\ntests/test_feather_gpu.py: {time.time() - _T0:.1f} s wall time")


LAYOUTS = {   # sf, LR canvas sizes, chop, stride
    "sf4": (4, [(40, 28), (12, 40)], 16, 12),
    "sf1": (1, [(13, 21), (8, 19)], 8, 5),          # canvas columns and origins that are no multiples of four: the scalar path
    "short": (4, [(3, 28), (40, 5)], 16, 12),       # tile sides shorter than two ramps
}


def _layout(name):
    from resshift_amd.tilepool import tile_windows

    sf, sizes, chop, stride = LAYOUTS[name]
    wins = [tile_windows(h, w, chop, stride) for h, w in sizes]
    order = [(0, k) for k in range(len(wins[0]))] + [(1, k) for k in range(len(wins[1]))]
    order = order[::2] + order[1::2]          # tiles of the two canvases interleaved, not in canvas order
    return sf, sizes, chop, stride, wins, order, R.ramp(chop, stride, sf)


def _canvases(sizes, sf, gpu):
    return [(torch.zeros(3, h * sf, w * sf, device=gpu), torch.zeros(h * sf, w * sf, device=gpu)) for h, w in sizes]


def _rows(canv, sizes, wins, order):
    return [(canv[i][0], canv[i][1], sizes[i][0], sizes[i][1], *wins[i][k]) for i, k in order]


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_weighted_scatter_equals_weighted_accumulate_tile_by_tile(gpu, layout):
    """one launch of overlapping tiles of two canvases == rs_tile_accumulate_weighted tile by tile in index order, counts included -
    also on canvases that already hold values (second launch)"""
    from resshift_amd import _lib

    sf, sizes, chop, stride, wins, order, Rr = _layout(layout)
    assert Rr == (3 if layout == "sf1" else 16)
    g = torch.Generator().manual_seed(61)
    n, P = len(order), chop * sf
    got, want = _canvases(sizes, sf, gpu), _canvases(sizes, sf, gpu)
    for launch in range(2):
        batch = torch.randn(n, 3, P, P, generator=g).to(gpu)
        _lib.tile_scatter(_rows(got, sizes, wins, order), batch, sf, ramp=(Rr, Rr))
        for r, (i, k) in enumerate(order):
            h0, w0, th, tw = wins[i][k]
            crop = batch[r:r + 1, :, :th * sf, :tw * sf].contiguous()
            _lib.tile_accumulate_weighted(want[i][0][None], want[i][1], crop, h0 * sf, w0 * sf, (Rr, Rr))
        torch.cuda.synchronize()
        for i in range(2):
            assert torch.equal(got[i][1], want[i][1]) and torch.equal(got[i][0], want[i][0]), (layout, launch, i)
    assert 0 < got[0][1].min().item() and got[0][1].max().item() <= 8   # weight sums now, no longer tile counts
    if layout == "short":   # the 12-row tiles never reach full weight: (5 + 0.5) / 16 per launch and tile at most
        assert got[0][1].max().item() <= 2 * 2 * 5.5 / 16


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_ramp_zero_is_the_unweighted_scatter(gpu, layout):
    from resshift_amd import _lib

    sf, sizes, chop, stride, wins, order, _ = _layout(layout)
    g = torch.Generator().manual_seed(62)
    n, P = len(order), chop * sf
    got, want = _canvases(sizes, sf, gpu), _canvases(sizes, sf, gpu)
    for launch in range(2):
        batch = torch.randn(n, 3, P, P, generator=g).to(gpu)
        _lib.tile_scatter(_rows(got, sizes, wins, order), batch, sf, ramp=(0, 0))
        _lib.tile_scatter(_rows(want, sizes, wins, order), batch, sf)
        torch.cuda.synchronize()
        for i in range(2):
            assert torch.equal(got[i][1], want[i][1]) and torch.equal(got[i][0], want[i][0]), (layout, launch, i)
    assert got[0][1].min().item() == 2 and got[0][1].max().item() == (4 if layout == "short" else 8)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_scatter_and_finalize_against_the_float64_restatement(gpu, layout):
    from resshift_amd import _lib

    sf, sizes, chop, stride, wins, order, Rr = _layout(layout)
    g = torch.Generator().manual_seed(63)
    n, P = len(order), chop * sf
    canv = _canvases(sizes, sf, gpu)
    ref = [[] for _ in sizes]
    for launch in range(2):
        batch = torch.rand(n, 3, P, P, generator=g) * 2 - 1
        _lib.tile_scatter(_rows(canv, sizes, wins, order), batch.to(gpu), sf, ramp=(Rr, Rr))
        for r, (i, k) in enumerate(order):
            h0, w0, th, tw = wins[i][k]
            ref[i].append((batch[r, :, :th * sf, :tw * sf].numpy(), h0 * sf, w0 * sf))
    worst = 0.0
    for i, (h, w) in enumerate(sizes):
        out = _lib.tile_finalize(*canv[i]).cpu().numpy().astype(np.float64)
        want = R.blend((3, h * sf, w * sf), ref[i], Rr, Rr)
        worst = max(worst, float(np.abs(out - want).max()))
    print(f"feather scatter + finalize, {layout} (sf {sf}, R = {Rr}): max |device - float64 restatement| = {worst:.3e} (bound {TOL:.0e})")
    assert worst <= TOL, worst


def test_seam_property_on_the_device(gpu):
    """two constant tiles, +1 and -1, chop 16 / stride 12 / sf 4 (R = 16, n = 64): the blend crosses the overlap as (R - 1 - 2p)/R, no
    neighbouring pixels differ by more than 2/R; the uniform average of the same tiles steps by 1"""
    from resshift_amd import _lib

    sf, Rr, n = 4, 16, 64
    batch = torch.stack([torch.full((3, n, n), 1.0), torch.full((3, n, n), -1.0)]).to(gpu)
    outs = {}
    for ramp in ((Rr, Rr), None):
        acc, cnt = torch.zeros(3, n, 112, device=gpu), torch.zeros(n, 112, device=gpu)
        _lib.tile_scatter([(acc, cnt, 16, 28, 0, 0, 16, 16), (acc, cnt, 16, 28, 0, 12, 16, 16)], batch, sf, ramp=ramp)
        outs[ramp] = _lib.tile_finalize(acc, cnt).cpu().double()
    out = outs[(Rr, Rr)]
    jump = max(out.diff(dim=2).abs().max().item(), out.diff(dim=1).abs().max().item())
    p = torch.arange(Rr, dtype=torch.float64)
    err = (out[:, :, 48:64] - (Rr - 1 - 2 * p) / Rr).abs().max().item()
    print(f"seam: max neighbour jump {jump:.6f} (2/R = {2 / Rr:.6f}), max |overlap - (R-1-2p)/R| = {err:.3e}")
    assert jump <= 2 / Rr + TOL and err <= TOL
    assert torch.all(out[:, :, :48] == 1) and torch.all(out[:, :, 64:] == -1)
    assert outs[None].diff(dim=2).abs().max().item() == 1.0


# ---------------------------------------------------------------------------------------------------------------- end to end
_SAMPLER = []
SEED = 20240607


def _sampler(chop_bs):
    """the tiny case under the parity policy, built with tile_blend="feather"; the tiling parameters are plain attributes"""
    from resshift_amd import ResShiftSampler
    from resshift_amd.config import ConfigNode

    up, ap, dp, _ = H.CASES["tiny"]
    if not _SAMPLER:
        usd, asd = H.weights(up, ap)
        cfg = ConfigNode(model=ConfigNode(target="models.unet.UNetModelSwin", ckpt_path=None, params=up),
                         diffusion=ConfigNode(target="models.script_util.create_gaussian_diffusion", params=dp),
                         autoencoder=ConfigNode(target="ldm.models.autoencoder.VQModelTorch", ckpt_path=None, params=ap))
        _SAMPLER.append(ResShiftSampler(cfg, sf=dp["sf"], seed=1, precision="parity", tile_blend="feather",
                                        state_dicts={"model": usd, "autoencoder": asd}))
    s = _SAMPLER[0]
    s.chop_size, s.chop_stride, s.chop_bs, s.padding_offset = 16, 12, chop_bs, 16
    assert s.tile_blend == "feather"
    return s, dp


def test_sample_tiled_feather_against_the_restatement_of_its_own_tiles(gpu):
    """the 40 x 28 fixture image, six tiles, chop_bs 1, seeded: the blended image against the float64 restatement fed with the tiles'
    own outputs - sample_func(crop, seeds=[(seed, j)]) at batch 1, which is what sample_tiled computes for tile j"""
    from resshift_amd.tilepool import tile_windows

    s, dp = _sampler(1)
    sf = dp["sf"]
    y = mt.tiled_inputs(dp["steps"])[0].to(gpu)
    assert tuple(y.shape) == (1, 3, 40, 28)
    out = s.sample_tiled(y, seed=SEED)
    wins = tile_windows(40, 28, 16, 12)
    assert len(wins) == 6
    tiles = []
    for j, (h0, w0, th, tw) in enumerate(wins):
        t = s.sample_func(y[:, :, h0:h0 + th, w0:w0 + tw].contiguous(), seeds=[(SEED, j)])
        assert tuple(t.shape) == (1, 3, th * sf, tw * sf) and t.abs().max().item() <= 1
        tiles.append((t[0].cpu().numpy(), h0 * sf, w0 * sf))
    Rr = R.ramp(16, 12, sf)
    want = R.blend((3, 40 * sf, 28 * sf), tiles, Rr, Rr)
    err = float(np.abs(out[0].cpu().numpy().astype(np.float64) - want).max())
    uni = float(np.abs(R.blend((3, 40 * sf, 28 * sf), tiles, 0, 0) - want).max())
    print(f"sample_tiled feather, tiny 40 x 28: max |device - restatement| = {err:.3e} (bound {TOL:.0e}); "
          f"the uniform average of the same tiles is {uni:.3e} away")
    assert err <= TOL, err


def test_pool_equals_sample_tiled_under_feather_when_the_image_is_one_batch(gpu):
    from resshift_amd.tilepool import TilePool

    s, dp = _sampler(6)
    y = mt.tiled_inputs(dp["steps"])[0].to(gpu)
    ref = s.sample_tiled(y, seed=SEED)
    tp = TilePool(s, max_batch=6, keep_log=True, seeded=True)
    assert tp.blend == "feather" and tp.ramp == (16, 16)
    rid = tp.submit(y, seed=SEED)
    out = tp.drain()
    torch.cuda.synchronize()
    assert list(out) == [rid] and all(len(b) == 6 for b in tp.batches) and len(tp.batches) == dp["steps"]
    assert torch.equal(out[rid], ref[0])

"""The tile pool on the GPU (tiny cases only; the file prints its wall time).

  * rs_tile_gather / rs_tile_scatter against torch and against rs_tile_accumulate, bit for bit;
  * engine against engine, exact: an image whose six tiles are one batch on both sides, TilePool vs sample_tiled;
  * mixed sizes, staggered submits: every image against oracle.sample_tiled with the same per-tile draws, the 40 x 28 one also against
    the reference's stored output (tests/golden/reference_tiled.npz) - the 60 dB of tests/test_engine_gpu.py's tiled tests;
  * inpainting (mask as fourth source plane) against the oracle, with the per-image path's figure on the same input beside it;
  * ResShiftSampler.inference(pool=True) on a folder of PNGs of different sizes.
"""
import os
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers as H
from oracle import make_golden_tiled as mt
from oracle import resshift_oracle as oc

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

_T0 = time.time()
_SAMPLERS = {}


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    yield
    print(f"\ntests/test_tilepool_gpu.py: {time.time() - _T0:.1f} s wall time")


def _sampler(tag, precision, chop_size, chop_stride, chop_bs, offset):
    """one sampler (engine, packed weights) per case and policy; the tiling parameters are plain attributes"""
    from resshift_amd import ResShiftSampler
    from resshift_amd.config import ConfigNode

    up, ap, dp, _ = H.CASES[tag]
    if (tag, precision) not in _SAMPLERS:
        usd, asd = H.weights(up, ap)
        cfg = ConfigNode(model=ConfigNode(target="models.unet.UNetModelSwin", ckpt_path=None, params=up),
                         diffusion=ConfigNode(target="models.script_util.create_gaussian_diffusion", params=dp),
                         autoencoder=ConfigNode(target="ldm.models.autoencoder.VQModelTorch", ckpt_path=None, params=ap))
        _SAMPLERS[(tag, precision)] = (ResShiftSampler(cfg, sf=dp["sf"], seed=1, precision=precision,
                                                       state_dicts={"model": usd, "autoencoder": asd}), usd, asd)
    s, usd, asd = _SAMPLERS[(tag, precision)]
    s.chop_size, s.chop_stride, s.chop_bs, s.padding_offset = chop_size, chop_stride, chop_bs, offset
    return s, usd, asd


# ---------------------------------------------------------------------------------------------------------------- kernels
def _gather_ref(src, h0, w0, th, tw, Hp, Wp):
    return F.pad(src[None, :, h0:h0 + th, w0:w0 + tw], (0, Wp - tw, 0, Hp - th), mode="reflect")[0]


@pytest.mark.parametrize("case", ["mask_aligned", "no_mask_odd_origins", "scalar_width"])
def test_tile_gather_equals_crop_pad_and_channel_split(gpu, case):
    from resshift_amd import _lib

    g = torch.Generator().manual_seed(21)
    if case == "mask_aligned":       # windows with and without padding, two source images, the mask as fourth plane
        a, b = torch.randn(4, 40, 28, generator=g).to(gpu), torch.randn(4, 12, 40, generator=g).to(gpu)
        tiles = [(a, 0, 0, 16, 16), (b, 0, 24, 12, 16), (a, 24, 12, 16, 16), (b, 0, 0, 12, 16), (a, 12, 12, 16, 16)]
        Hp, Wp = 16, 16
    elif case == "no_mask_odd_origins":   # rows and origins that break the 16-byte alignment of the source, padding on both sides
        a, b = torch.randn(3, 23, 31, generator=g).to(gpu), torch.randn(3, 14, 13, generator=g).to(gpu)
        tiles = [(a, 5, 7, 14, 13), (b, 0, 0, 14, 13), (a, 9, 18, 14, 13), (a[:, 1:, :].contiguous(), 0, 1, 14, 13)]
        Hp, Wp = 16, 16
    else:                            # a padded width that is no multiple of four
        a, b = torch.randn(3, 11, 18, generator=g).to(gpu), torch.randn(3, 7, 40, generator=g).to(gpu)
        tiles = [(a, 1, 3, 7, 13), (b, 0, 27, 7, 13), (a, 4, 5, 7, 13)]
        Hp, Wp = 12, 18
    C = tiles[0][0].shape[0]
    out_lq = torch.full((len(tiles), 3, Hp, Wp), float("nan"), device=gpu)
    out_mask = torch.full((len(tiles), 1, Hp, Wp), float("nan"), device=gpu) if C == 4 else None
    _lib.tile_gather(tiles, out_lq, out_mask)
    torch.cuda.synchronize()
    for k, (src, h0, w0, th, tw) in enumerate(tiles):
        want = _gather_ref(src, h0, w0, th, tw, Hp, Wp)
        assert torch.equal(out_lq[k], want[:3].contiguous()), (case, k)
        if C == 4:
            assert torch.equal(out_mask[k], want[3:].contiguous()), (case, k)


@pytest.mark.parametrize("sf", [4, 1])
def test_tile_scatter_equals_accumulate_tile_by_tile(gpu, sf):
    """one launch holding overlapping tiles of two canvases (the four tiles around (12, 12) of the 40 x 28 canvas overlap four-fold) ==
    rs_tile_accumulate tile by tile in index order, counts included - also on canvases that already hold values (second launch)"""
    from resshift_amd import _lib
    from resshift_amd.tilepool import tile_windows

    lib = _lib.load()
    g = torch.Generator().manual_seed(22)
    if sf == 4:
        sizes, chop, stride = [(40, 28), (12, 40)], 16, 12
    else:            # canvas columns and origins that are no multiples of four: the scalar path
        sizes, chop, stride = [(13, 21), (8, 19)], 8, 5
    wins = [tile_windows(h, w, chop, stride) for h, w in sizes]
    order = [(0, k) for k in range(len(wins[0]))] + [(1, k) for k in range(len(wins[1]))]
    order = order[::2] + order[1::2]          # tiles of the two canvases interleaved, not in canvas order
    n, P = len(order), chop * sf
    ov = torch.zeros(sizes[0])
    for h0, w0, th, tw in wins[0]:
        ov[h0:h0 + th, w0:w0 + tw] += 1
    assert ov.max() == 4
    got = [(torch.zeros(3, h * sf, w * sf, device=gpu), torch.zeros(h * sf, w * sf, device=gpu)) for h, w in sizes]
    want = [(a.clone(), c.clone()) for a, c in got]
    st = _lib.current_stream_ptr()
    for launch in range(2):
        batch = torch.randn(n, 3, P, P, generator=g).to(gpu)
        _lib.tile_scatter([(got[i][0], got[i][1], sizes[i][0], sizes[i][1], *wins[i][k]) for i, k in order], batch, sf)
        for r, (i, k) in enumerate(order):
            h0, w0, th, tw = wins[i][k]
            crop = batch[r:r + 1, :, :th * sf, :tw * sf].contiguous()
            _lib.check(lib.rs_tile_accumulate(want[i][0].data_ptr(), want[i][1].data_ptr(), crop.data_ptr(), 1, 3, sizes[i][0] * sf,
                                              sizes[i][1] * sf, h0 * sf, w0 * sf, th * sf, tw * sf, st), "rs_tile_accumulate")
        torch.cuda.synchronize()
        for i in range(2):
            assert torch.equal(got[i][1], want[i][1]) and torch.equal(got[i][0], want[i][0]), (sf, launch, i)
    assert got[0][1].max().item() == 8 and got[0][1].min().item() == 2


# ---------------------------------------------------------------------------------------------------------------- engine vs engine
def _fixture_tile_noises(calls, dev):
    """the fixture's per-call noises (chop_bs 2) as per-tile draws: tile 2k + j = row j of call k"""
    return [(c[0][j:j + 1].to(dev), [n[j:j + 1].to(dev) for n in c[1:]]) for c in calls for j in range(c[0].shape[0])]


def test_pool_equals_sample_tiled_when_the_image_is_one_batch(gpu):
    from resshift_amd.tilepool import TilePool

    _, _, dp, _ = H.CASES["tiny"]
    s, _, _ = _sampler("tiny", "parity", 16, 12, 6, 16)
    y, calls = mt.tiled_inputs(dp["steps"])
    per_tile = _fixture_tile_noises(calls, gpu)
    assert len(per_tile) == 6
    one_call = [(torch.cat([t[0] for t in per_tile]), [torch.cat([t[1][k] for t in per_tile]) for k in range(dp["steps"])])]
    ref = s.sample_tiled(y.to(gpu), tile_noises=one_call)
    tp = TilePool(s, max_batch=6, keep_log=True)
    rid = tp.submit(y.to(gpu), tile_noises=per_tile)
    out = tp.drain()
    torch.cuda.synchronize()
    assert list(out) == [rid] and all(len(b) == 6 for b in tp.batches) and len(tp.batches) == dp["steps"]
    assert torch.equal(out[rid], ref[0])


# ---------------------------------------------------------------------------------------------------------------- vs the oracle
_ORACLE = {}


def _mixed_inputs():
    """the 40 x 28 fixture image with the fixture's draws per tile, a seeded 12 x 40 image (three cropped tiles of the padded class
    16 x 16) and a seeded 13 x 10 image (one tile); per image: (y [1,3,H,W], per-tile draw lists [steps+1 tensors [1,3,16,16]])"""
    _, _, dp, _ = H.CASES["tiny"]
    T = dp["steps"]
    y0, calls = mt.tiled_inputs(T)
    ims = [(y0, [[n[j:j + 1] for n in c] for c in calls for j in range(c[0].shape[0])])]
    g = torch.Generator().manual_seed(31)
    for (h, w), n_tiles in (((12, 40), 3), ((13, 10), 1)):
        y = torch.rand(1, 3, h, w, generator=g) * 2 - 1
        ims.append((y, [[torch.randn(1, 3, 16, 16, generator=g) for _ in range(T + 1)] for _ in range(n_tiles)]))
    return ims


def _mixed_oracle():
    if "mixed" not in _ORACLE:
        up, ap, dp, _ = H.CASES["tiny"]
        usd, asd = H.weights(up, ap)
        ims = _mixed_inputs()
        _ORACLE["mixed"] = (ims, [oc.sample_tiled(usd, up, asd, ap, dp, y, draws, chop_size=16, chop_stride=12, chop_bs=1, padding_offset=16)
                                  for y, draws in ims])
    return _ORACLE["mixed"]


@pytest.mark.parametrize("policy", ["fp32", "parity"])
def test_pool_mixed_sizes_staggered_vs_oracle_and_reference_output(gpu, policy):
    from resshift_amd.tilepool import TilePool

    s, _, _ = _sampler("tiny", policy, 16, 12, 1, 16)
    ims, refs = _mixed_oracle()
    tp = TilePool(s, max_batch=4, keep_log=True)
    arrivals, ids, out, k = {0: 0, 1: 1, 3: 2}, {}, {}, 0
    while k < 4 or tp.pending():
        if k in arrivals:
            y, draws = ims[arrivals[k]]
            ids[tp.submit(y.to(gpu), tile_noises=[(d[0].to(gpu), [n.to(gpu) for n in d[1:]]) for d in draws])] = arrivals[k]
        out.update(tp.step())
        k += 1
    torch.cuda.synchronize()
    assert sorted(out) == sorted(ids) and len(ids) == 3
    gold = torch.from_numpy(np.load(os.path.join(H.ROOT, "tests", "golden", "reference_tiled.npz"))["sample"])
    for rid, i in ids.items():
        assert tuple(out[rid].shape) == tuple(refs[i].shape[1:])
        p = H.psnr(out[rid].cpu(), refs[i][0])
        print(f"tile pool {policy}, image {i} {tuple(ims[i][0].shape[2:])}: PSNR {p:.1f} dB vs oracle.sample_tiled")
        assert p >= 60.0, (i, p)
        if i == 0:
            pg = H.psnr(out[rid].cpu(), gold[0])
            print(f"tile pool {policy}, image 0: PSNR {pg:.1f} dB vs the reference output")
            assert pg >= 60.0
    assert any(len({i for i, _ in b}) > 1 for b in tp.batches), tp.batches   # tiles of two images in one engine step
    assert max(len(b) for b in tp.batches) <= 4


def _oracle_tiled_masked(usd, up, asd, ap, dp, im_lq, tile_noises, mask, chop_size, chop_stride, padding_offset):
    """oracle.sample_tiled(..., mask=..., chop_bs=1) line by line, with ONE difference: oracle.sample_func restates the reference, which
    reflect-pads the LR tile only (sampler.py:130-138) and then fails in the UNet's channel concat when a masked tile needs padding;
    ResShiftSampler.sample_func pads the mask alike (its documented deviation), and so does this.  Where no tile needs padding this IS
    oracle.sample_tiled (pinned in the test below)."""
    sf = int(dp.get("sf", 4))
    B, _, Hh, W = im_lq.shape
    x = torch.cat([im_lq, mask], dim=1)
    starts = [(i, j) for i in oc.tile_starts(Hh, chop_size, chop_stride) for j in oc.tile_starts(W, chop_size, chop_stride)]
    res = count = None
    for k, (h0, w0) in enumerate(starts):
        pch = x[:, :, h0:h0 + chop_size, w0:w0 + chop_size]
        th, tw = pch.shape[2:]
        ph, pw = -(-th // padding_offset) * padding_offset - th, -(-tw // padding_offset) * padding_offset - tw
        if ph or pw:
            pch = F.pad(pch, (0, pw, 0, ph), mode="reflect")
        out = oc.sample_loop(usd, up, asd, ap, dp, pch[:, :-1], tile_noises[k], mask=pch[:, -1:])[:, :, :th * sf, :tw * sf].clamp_(-1.0, 1.0)
        if res is None:
            res = torch.zeros(B, out.shape[1], Hh * sf, W * sf)
            count = torch.zeros_like(res)
        res[:, :, h0 * sf:(h0 + chop_size) * sf, w0 * sf:(w0 + chop_size) * sf] += out
        count[:, :, h0 * sf:(h0 + chop_size) * sf, w0 * sf:(w0 + chop_size) * sf] += 1
    assert torch.all(count != 0)
    return res / count


def test_pool_inpainting_mask_travels_as_fourth_plane(gpu):
    """tiny_fe (mask-conditioned, sf = 1): an 80 x 52 image at chop 64 / stride 48 / padding_offset 64 - two 64 x 52 tiles, padded to
    64 x 64 - through the pool and through the per-image path, both against the oracle at the per-image path's 60 dB."""
    from resshift_amd.tilepool import TilePool

    up, ap, dp, with_mask = H.CASES["tiny_fe"]
    assert with_mask and dp["sf"] == 1
    s, usd, asd = _sampler("tiny_fe", "parity", 64, 48, 1, 64)
    T = dp["steps"]
    g = torch.Generator().manual_seed(41)
    y = torch.rand(1, 3, 80, 52, generator=g) * 2 - 1
    mask = (torch.rand(1, 1, 80, 52, generator=g) > 0.5).float() * 2 - 1
    draws = [[torch.randn(1, 3, 16, 16, generator=g) for _ in range(T + 1)] for _ in range(2)]
    # the restatement above is oracle.sample_tiled where the oracle can run (no padding): 80 x 64, one draw set reused
    y_np, m_np = F.pad(y, (0, 12, 0, 0), mode="reflect"), F.pad(mask, (0, 12, 0, 0), mode="reflect")
    pin = oc.sample_tiled(usd, up, asd, ap, dp, y_np, draws, mask=m_np, chop_size=64, chop_stride=48, chop_bs=1, padding_offset=64)
    assert torch.equal(pin, _oracle_tiled_masked(usd, up, asd, ap, dp, y_np, draws, m_np, 64, 48, 64))
    ref = _oracle_tiled_masked(usd, up, asd, ap, dp, y, draws, mask, 64, 48, 64)
    tn = [(d[0].to(gpu), [n.to(gpu) for n in d[1:]]) for d in draws]
    per_image = s.sample_tiled(y.to(gpu), mask=mask.to(gpu), tile_noises=tn)
    tp = TilePool(s, max_batch=4)
    rid = tp.submit(y.to(gpu), mask=mask.to(gpu), tile_noises=tn)
    out = tp.drain()
    torch.cuda.synchronize()
    assert tuple(out[rid].shape) == (3, 80, 52) == tuple(ref.shape[1:])
    p_img, p_pool = H.psnr(per_image.cpu(), ref), H.psnr(out[rid].cpu(), ref[0])
    print(f"inpainting 80 x 52: per-image path {p_img:.1f} dB, tile pool {p_pool:.1f} dB vs the oracle")
    assert p_img >= 60.0 and p_pool >= 60.0


# ---------------------------------------------------------------------------------------------------------------- inference
def test_inference_pool_on_a_folder_of_different_sizes(gpu, tmp_path):
    from PIL import Image

    from resshift_amd.tilepool import TilePool

    s, _, _ = _sampler("tiny", "parity", 16, 12, 1, 16)
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    g = torch.Generator().manual_seed(51)
    sizes = {"a": (40, 28), "b": (12, 40), "c": (13, 10)}
    for name, (h, w) in sizes.items():
        Image.fromarray((torch.rand(h, w, 3, generator=g) * 255).to(torch.uint8).numpy()).save(src / f"{name}.png")
    s.setup_seed()
    s.inference(src, dst, bs=3, pool=True)
    got = {name: np.asarray(Image.open(dst / f"{name}.png")) for name in sizes}
    assert sorted(p.name for p in dst.iterdir()) == ["a.png", "b.png", "c.png"]
    s.setup_seed()
    tp = TilePool(s)
    ids = {}
    for name in sorted(sizes):
        lq = s.engine.u8_to_input(s._read_image_u8(src / f"{name}.png").unsqueeze(0).to(gpu))
        ids[tp.submit(lq)] = name
    for rid, img in tp.drain().items():
        name = ids[rid]
        want = s.engine.output_to_u8(img.unsqueeze(0))[0].cpu().numpy()
        assert got[name].shape == (sizes[name][0] * 4, sizes[name][1] * 4, 3) == want.shape and got[name].dtype == np.uint8
        assert np.array_equal(got[name], want), name
    with pytest.raises(RuntimeError, match="stack"):   # unchanged: the per-image path stacks a batch, so sizes must agree
        s.inference(src, tmp_path / "out2", bs=3)

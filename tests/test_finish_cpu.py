"""The finishing stage (resshift_amd/finish.py) without a GPU and without the library: what `Finish.of` reads from a sampler, the order of
its two engine calls, the texts of `reject_mask`, and that every route a whole image can take - `sample_tiled`, the `TilePool`, `inference`
with and without the pool - goes through it once per image and never per tile."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401  (puts the repository root on sys.path)
from _fakes import FakeEngine, _OnDevice, fake_launches, fake_sampler  # noqa: F401  (fixtures)
from resshift_amd import _lib, tiling
from resshift_amd.finish import Finish
from resshift_amd.sampler import ResShiftSampler
from resshift_amd.tilepool import TilePool


def test_of_reads_the_sampler_and_defaults_what_it_lacks():
    assert Finish.of(SimpleNamespace(sf=4)) == Finish(4, "uniform", "none", None, None)
    assert Finish.of(SimpleNamespace()) == Finish(None, "uniform", "none", None, None)          # no out_scale: no sf is needed
    full = SimpleNamespace(sf=4, tile_blend="feather", color_fix="adain", out_scale=2)
    assert Finish.of(full) == Finish(4, "feather", "adain", 2, 2)
    assert Finish.of(full, sf=2) == Finish(2, "feather", "adain", 2, None)                      # the caller's sf wins (TilePool: the diffusion's)
    for same in (4, 4.0):   # the raw value is kept, the effective one is None
        f = Finish.of(SimpleNamespace(sf=4, out_scale=same))
        assert f.out_scale == same and type(f.out_scale) is type(same) and f.resize_to is None
    assert Finish.of(SimpleNamespace(sf=4, out_scale=0.7)).resize_to == 0.7
    for bad, text in ((dict(tile_blend="gauss"), "unknown tile blend 'gauss'"), (dict(color_fix="ycbcr"), "unknown colour fix 'ycbcr'"),
                      (dict(color_fix=None), "unknown colour fix"), (dict(out_scale="2"), "out_scale must be None or a positive number"),
                      (dict(out_scale=True), "out_scale must be None or a positive number"), (dict(out_scale=40), "is outside")):
        with pytest.raises(ValueError, match=text):
            Finish.of(SimpleNamespace(sf=4, **bad))


@pytest.mark.parametrize("fix", ["none", "wavelet", "adain"])
@pytest.mark.parametrize("out_scale", [None, 4, 4.0, 2, 0.7])
def test_call_fixes_then_resizes_each_at_most_once(fix, out_scale):
    eng = FakeEngine()
    sr, lq = torch.zeros(2, 3, 40, 28), torch.zeros(2, 3, 10, 7)
    out = Finish.of(SimpleNamespace(sf=4, color_fix=fix, out_scale=out_scale))(eng, sr, lq)
    want = [("color_fix", (2, 3, 40, 28), fix)] if fix != "none" else []
    if out_scale in (2, 0.7):   # the resize sees the fixed image (minimum 1) and the size comes from lq
        size = tiling.out_size(10, 7, out_scale)
        want.append(("resize", (2, 3, 40, 28), 1.0 if fix != "none" else 0.0, None, size, True))
        assert tuple(out.shape) == (2, 3, *size)
    assert eng.calls == want
    if not want:
        assert out is sr                                           # no engine call, the same tensor object
    elif out_scale not in (2, 0.7):
        assert torch.equal(out, sr + 1.0) and torch.equal(eng.fixes[0][1], lq)


def test_reject_mask_gives_the_six_texts():
    texts = {
        "sample_tiled": ("color_fix='wavelet' is undefined for a masked input (the LQ image has a hole): use color_fix='none'",
                         "out_scale=2 is undefined for a masked input (lq and mask stay at the model's size): use out_scale=None"),
        "inference": ("color_fix='wavelet' is undefined for masked (inpainting) inputs: use color_fix='none'",
                      "out_scale=2 is undefined for masked (inpainting) inputs: use out_scale=None"),
        "TilePool": ("color_fix='wavelet' is undefined for a model conditioned on a mask (the LQ image has a hole)",
                     "out_scale=2 is undefined for a model conditioned on a mask (lq and mask stay at the model's size)"),
    }
    for context, (fix_text, scale_text) in texts.items():
        for f, text in ((Finish(4, "uniform", "wavelet", None, None), fix_text), (Finish(4, "uniform", "none", 2, 2), scale_text),
                        (Finish(4, "uniform", "wavelet", 2, 2), fix_text)):                       # the colour fix is named first
            with pytest.raises(ValueError) as e:
                f.reject_mask(context)
            assert str(e.value) == text
        Finish(4, "feather", "none", 4, None).reject_mask(context)                                # nothing to finish: a mask is fine


# ---------------------------------------------------------------------------------------------------------------- every route, once per image
@pytest.fixture
def recorder(monkeypatch, fake_launches):
    """Finish.__call__ replaced by a recorder, the library's tile launches by torch restatements"""
    seen = []
    monkeypatch.setattr(Finish, "__call__", lambda self, engine, sr, lq: seen.append((tuple(sr.shape), tuple(lq.shape))) or sr)
    monkeypatch.setattr(_lib, "load", lambda: SimpleNamespace(rs_tile_accumulate=lambda *a: 0, rs_tile_finalize=lambda *a: 0))
    monkeypatch.setattr(_lib, "window_copy", lambda x, h0, w0, ho, wo, out=None: out.copy_(x[..., h0:h0 + ho, w0:w0 + wo]))
    return seen


class _FileEngine(FakeEngine):
    """the engine of the file loop: uint8 HWC in, uint8 HWC out, on tensors that pass for device tensors"""

    def u8_to_input(self, t):
        return (t.permute(0, 3, 1, 2).float() / 255).as_subclass(_OnDevice)

    def output_to_u8(self, sr, lq=None, mask=None):
        return torch.zeros(sr.shape[0], sr.shape[2], sr.shape[3], 3, dtype=torch.uint8)


def _sampler(**extra):
    """a ResShiftSampler over the stand-in's parts, with a sample_func that counts the tiles it is given"""
    s = ResShiftSampler.__new__(ResShiftSampler)
    s.__dict__.update(fake_sampler(engine=_FileEngine(), **extra).__dict__)
    s.sf, s.chop_bs, s.rank, s.num_gpus, s.tiles = 4, 2, 0, 1, 0

    def sample_func(pch, noise_repeat=False, mask=None, noise=None, step_noises=None, seeds=None):
        s.tiles += pch.shape[0]
        return torch.zeros(pch.shape[0], 3, pch.shape[2] * 4, pch.shape[3] * 4)

    s.sample_func = sample_func
    return s


@pytest.mark.parametrize("size,tiles", [((40, 28), 6), ((16, 12), 1)], ids=["tiled", "untiled"])
def test_sample_tiled_finishes_the_image_it_returns_once(recorder, size, tiles):
    s = _sampler(color_fix="wavelet", out_scale=2)
    s.sample_tiled(torch.zeros(1, 3, *size).as_subclass(_OnDevice), seed=3)
    assert s.tiles == tiles and recorder == [((1, 3, size[0] * 4, size[1] * 4), (1, 3, *size))]


def test_tile_pool_finishes_each_completed_image_once(recorder):
    tp = TilePool(fake_sampler(tile_blend="feather", color_fix="adain", out_scale=3), max_batch=4, seeded=True)
    assert (tp.blend, tp.ramp, tp.color_fix, tp.out_scale) == ("feather", (16, 16), "adain", 3)
    sizes = [(40, 28), (13, 10), (12, 40)]          # six tiles, one whole image, three cropped tiles
    for Hh, W in sizes:
        tp.submit(torch.zeros(3, Hh, W))
    out = tp.drain()
    assert sorted(out) == [0, 1, 2]
    assert sorted(recorder) == sorted(((1, 3, 4 * Hh, 4 * W), (1, 3, Hh, W)) for Hh, W in sizes)   # lq: the image's own planes


@pytest.mark.parametrize("pool", [False, True])
def test_inference_finishes_each_file_once(recorder, tmp_path, pool):
    from PIL import Image

    src = tmp_path / "in"
    src.mkdir()
    sizes = {"a": (40, 28), "b": (16, 12), "c": (40, 28)}
    for name, (Hh, W) in sizes.items():
        Image.fromarray(np.zeros((Hh, W, 3), dtype=np.uint8)).save(src / f"{name}.png")
    s = _sampler(color_fix="wavelet")
    assert s.inference(src, tmp_path / "out", bs=1, pool=pool, seeded=True) is None
    assert sorted(recorder) == sorted(((1, 3, 4 * Hh, 4 * W), (1, 3, Hh, W)) for Hh, W in sizes.values())
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["a.png", "b.png", "c.png"]
    assert pool or s.tiles == 6 + 1 + 6

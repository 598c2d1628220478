"""What the host-plumbing tests share: the library fixture, a CPU tensor that passes for a device tensor, the passive engine of the
whole-image features, the stand-in sampler every scheduler test builds its pools on and torch restatements of the pool's launches.  The
recording engines of tests/test_continuous_cpu.py, test_tilepool_cpu.py and test_noise_cpu.py stay in their files - their records and
in-engine asserts are what those files check - and pass themselves in."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import helpers  # noqa: F401  (puts the repository root on sys.path)
from oracle import cases
from resshift_amd import _lib, build
from resshift_amd.gaussian_diffusion import create_gaussian_diffusion


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


class _OnDevice(torch.Tensor):
    """a CPU tensor that says it is a device tensor: TileSplitter and the _lib wrappers refuse host tensors, and their kernels are faked"""
    is_cuda = True


class FakeEngine:
    """Stands in for resshift_amd.engine.Engine, with and without keys: x[:, 0, 0, 0] carries a tile's code (the top-left pixel of its LR
    window) and the decoded tile is its code everywhere.  The colour fix adds one; the resize returns a tensor of the asked size filled
    with the input's first value plus ten.  Both are recorded: `calls` holds ("color_fix", shape, mode) and ("resize", shape, min, scale,
    size, clamp) in call order, `fixes` (shape, the lq the fix saw, mode)."""

    def __init__(self):
        self.calls, self.fixes = [], []

    def latent_shape(self, B, h, w, sf):
        return (B, 3, h * sf // 4, w * sf // 4)

    def film_prewarm(self, timesteps):
        pass

    def sample_begin(self, y, noise, tables, sf, scale_factor, prec_encode=None, out=None, keys=None):
        out.zero_()
        out[:, 0, 0, 0] = y[:, 0, 0, 0]
        return out

    def sample_step(self, x, y, t, noise, tables, sf, mask=None, prec=None, pred_xstart=None, keys=None):
        return x

    def sample_end(self, x0, h, w, sf, scale_factor, prec_decode=None, return_aux=False):
        return x0[:, 0, 0, 0].view(-1, 1, 1, 1).expand(-1, 3, h * sf, w * sf).contiguous() * 1.0

    def color_fix(self, sr, lq, mode="wavelet"):
        self.calls.append(("color_fix", tuple(sr.shape), mode))
        self.fixes.append((tuple(sr.shape), lq.clone(), mode))
        return sr + 1.0

    def resize(self, x, scale=None, size=None, clamp=False):
        self.calls.append(("resize", tuple(x.shape), float(x.min()), scale, size, clamp))
        return torch.full((x.shape[0], x.shape[1], *size), float(x.flatten()[0]) + 10.0)


def fake_sampler(cond_mask=False, precision=("split", "split", "fp16"), autoencoder=True, chop_size=16, chop_stride=12, offset=16, seed=77,
                 engine=None, **extra):
    """what ContinuousSampler and TilePool read from a built ResShiftSampler, over TINY_DIFFUSION (sf = 4, four steps); `engine`: a
    recording engine of the caller's (default: a FakeEngine); `extra`: the options a sampler may or may not have (tile_blend, ...)"""
    d = create_gaussian_diffusion(**cases.TINY_DIFFUSION)
    d.set_precision(*precision)
    return SimpleNamespace(base_diffusion=d, engine=engine if engine is not None else FakeEngine(), autoencoder=object() if autoencoder else None,
                           padding_offset=offset, chop_size=chop_size, chop_stride=chop_stride, seed=seed,
                           configs={"model": {"params": {"cond_mask": cond_mask}}}, device=torch.device("cpu"), **extra)


@pytest.fixture
def fake_launches(monkeypatch):
    """torch restatements of the pool's three launches under the uniform blend"""
    def gather(tiles, out_lq, out_mask=None):
        Hp, Wp = out_lq.shape[-2:]
        for k, (src, h0, w0, th, tw) in enumerate(tiles):
            out_lq[k] = F.pad(src[None, :3, h0:h0 + th, w0:w0 + tw], (0, Wp - tw, 0, Hp - th), mode="reflect")[0]

    def scatter(tiles, batch, sf, ramp=None):
        for k, (acc, cnt, Hh, W, h0, w0, th, tw) in enumerate(tiles):
            acc[:, h0 * sf:(h0 + th) * sf, w0 * sf:(w0 + tw) * sf] += batch[k, :, :th * sf, :tw * sf]
            cnt[h0 * sf:(h0 + th) * sf, w0 * sf:(w0 + tw) * sf] += 1

    monkeypatch.setattr(_lib, "tile_gather", gather)
    monkeypatch.setattr(_lib, "tile_scatter", scatter)
    monkeypatch.setattr(_lib, "tile_finalize", lambda acc, count: acc.div_(count))


class InstantPool:
    """tilepool.TilePool as `inference(pool=True)` drives it: every image completes at the next step, as `finished(lq, seed)`"""

    def __init__(self, sampler, seeded=False):
        self.seeded, self.done, self.n = seeded, {}, 0

    def finished(self, lq, seed):
        return lq[0]          # the "sample" is the input

    def submit(self, lq, mask=None, seed=None):
        self.done[self.n] = self.finished(lq, seed)
        self.n += 1
        return self.n - 1

    def waiting_tiles(self):
        return 0

    def pending(self):
        return len(self.done)

    def step(self):
        d, self.done = self.done, {}
        return d

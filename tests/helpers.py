"""Shared test helpers: synthetic weights keyed by the product's specs, golden fixtures, metrics."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import cases, synth  # noqa: E402
from resshift_amd.config import load_config, to_plain  # noqa: E402
from resshift_amd.spec import ae_param_spec, unet_param_spec  # noqa: E402

SEED_W, SEED_X = 1, 123
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_outputs.npz")

CASES = {
    "tiny": (cases.TINY_UNET, cases.TINY_AE, cases.TINY_DIFFUSION, False),
    "tiny_fe": (cases.TINY_UNET_FE, cases.TINY_AE, cases.TINY_DIFFUSION_SF1, True),
    "tiny_fe8": (cases.TINY_UNET_FE8, cases.TINY_AE8, cases.TINY_DIFFUSION_SF1, False),
}


def golden():
    return np.load(GOLDEN)


def realsr_params():
    cfg = to_plain(load_config("realsr_swinunet_realesrgan256"))
    return cfg["model"]["params"], cfg["autoencoder"]["params"], cfg["diffusion"]["params"]


def weights(unet_p, ae_p):
    uspec, _ = unet_param_spec(unet_p)
    usd = synth.synthetic_state_dict(uspec, SEED_W, image_size=unet_p["image_size"])
    asd = synth.synthetic_state_dict(ae_param_spec(ae_p), SEED_W)
    return usd, asd


def case_inputs(unet_p, ae_p, dp, with_mask, B=2):
    sf, steps = dp["sf"], dp["steps"]
    hz = unet_p["image_size"]
    h = hz * 4 // sf
    return synth.synthetic_inputs(SEED_X, B, h, h, ae_p["embed_dim"], hz, hz, steps, with_mask=with_mask)


def psnr(a, b, peak_to_peak=2.0):
    mse = torch.mean((a.double() - b.double()) ** 2).item()
    return float("inf") if mse == 0 else 10.0 * math.log10(peak_to_peak ** 2 / mse)


def rel_err(got, ref):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    return (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-12)


# ---- the VQ step of the autoencoder block tests (test_ae_blocks_cpu.py / test_ae_blocks_gpu.py)
VQ_CAP = 1e-3   # share of an image's positions whose index may differ from the float64 argmin


def vq_latents(B, C, h, w, seed):
    """decoder inputs of the autoencoder block tests: noise of scale 0.7 (not codebook rows: every position has a real runner-up)"""
    return torch.randn(B, C, h, w, generator=torch.Generator().manual_seed(seed)) * 0.7


def vq_check(z64, e64, idx):
    """One image's VQ indices `idx` [h*w] against float64 distances recomputed from its latents z64 [1,C,h,w] and the codebook e64 [n,C]
    (the three-term expression of ldm/modules/vqvae/quantize.py:276-285 in float64).  An index is right when it is the float64 argmin, or
    when its float64 distance exceeds the minimum by no more than 8 * 2^-23 * (|z|^2 + max |e|^2): a few fp32 roundings of that
    expression, which the reference itself evaluates in fp32.  Returns (share of positions whose index is not the float64 argmin, number of
    positions whose index is wrong, float64 index tensor)."""
    zf = z64.permute(0, 2, 3, 1).reshape(-1, e64.shape[1])
    ee = torch.sum(e64 ** 2, dim=1)
    d = torch.sum(zf ** 2, dim=1, keepdim=True) + ee - 2 * zf @ e64.t()
    dmin, ref = d.min(dim=1)
    idx = idx.reshape(-1).long()
    assert idx.numel() == zf.shape[0] and int(idx.min()) >= 0 and int(idx.max()) < e64.shape[0], "VQ index out of the codebook"
    excess = d.gather(1, idx[:, None])[:, 0] - dmin
    slack = 8 * 2.0 ** -23 * (torch.sum(zf ** 2, dim=1) + ee.max())
    differ = idx != ref
    return differ.double().mean().item(), int((differ & (excess > slack)).sum()), ref

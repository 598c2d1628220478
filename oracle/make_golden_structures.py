"""Golden vectors for network STRUCTURES other than the two the other fixtures build (oracle/cases.py: STRUCTURES): one-level nets, levels
without a skip conv, unequal block counts, channel_mult[0] != 1, levels without Swin, odd and single swin_depth, a hidden size off a
multiple of 64, 3 channels per GroupNorm group, one feature-extractor stage with a mask, E = 192 / 6 heads off model_channels 160;
autoencoders with one level, with equal neighbours in ch_mult, z_channels != embed_dim and a 4-dimensional codebook.

Produced by the UNMODIFIED reference modules (imported from /root/reference) on synthetic weights (oracle/synth.py, SEED_W) loaded with a
strict load_state_dict; the oracle restatement is asserted against every output in the same run (2e-5 of the output's scale; VQ indices
all equal).  Stored in tests/golden/reference_structures.npz:

  unet/<tag>            one forward at B = 2, timesteps 1 and 3, at the constructed size (fp32)
  ae/<tag>/encode       the latent of a 2 x 3 x 32 x 32 batch (ae_f1: 16 x 16)            (fp32)
  ae/<tag>/decode, decode_idx   the image and the VQ indices of a latent of that size    (fp32, int32)
  pair/<tag>/sample, sample_z, sample_idx   the 4-step loop at B = 2 (the image as fp16 where it is 128 x 128: it is compared in dB)
  keys/unet/<tag>, keys/ae/<tag>   the reference's state_dict: names and shapes, no values (JSON)

    python -m oracle.make_golden_structures        (build container only: needs /root/reference)
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import cases, ref_import, resshift_oracle as oc, synth  # noqa: E402
from oracle.make_golden import SEED_W, check, ref_sample  # noqa: E402
from resshift_amd.spec import ae_param_spec, unet_param_spec  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
PATH = os.path.join(GOLD, "reference_structures.npz")
SEED_X = 555
T_UNET = (1, 3)   # the two timesteps of a structure's UNet forward
S = cases.STRUCTURES


def unet_weights(up):
    return synth.synthetic_state_dict(unet_param_spec(up)[0], SEED_W, image_size=up["image_size"])


def ae_weights(ap):
    return synth.synthetic_state_dict(ae_param_spec(ap), SEED_W)


def ae_factor(ap):
    return 2 ** (len(ap["ddconfig"]["ch_mult"]) - 1)


def unet_inputs(tag):
    """(x, t, kwargs) of a UNet structure's forward: B = 2 at the constructed size, two different timesteps"""
    up = S["unet"][tag]
    hz, hl = int(up["image_size"]), int(up["lq_size"])
    with_mask = bool(up.get("cond_mask"))
    y, noises, mask = synth.synthetic_inputs(SEED_X, 2, hl, hl, int(up["in_channels"]), hz, hz, 1, with_mask=with_mask)
    kw = {"lq": y}
    if with_mask:
        kw["mask"] = mask
    return noises[1] * 1.3, torch.tensor(T_UNET), kw


def ae_inputs(tag):
    """(image batch, latent batch) of an autoencoder structure: 2 x 3 x 32 x 32 (ae_f1: 16 x 16) and a latent of the size it encodes to"""
    ap = S["ae"][tag]
    side = 16 if tag == "ae_f1" else 32
    g = np.random.Generator(np.random.PCG64(11))
    img = torch.from_numpy(g.random((2, 3, side, side), dtype=np.float32) * 2 - 1)
    z = torch.from_numpy(g.standard_normal((2, int(ap["embed_dim"]), side // ae_factor(ap), side // ae_factor(ap)), dtype=np.float32)) * 0.8
    return img, z


def pair_inputs(tag):
    """(y, noises, mask) of a pair's 4-step loop at B = 2: the LR side gives a latent of the UNet's constructed size"""
    up, ap, dp, with_mask = cases.structure_pair(tag)
    hz = int(up["image_size"])
    lr = hz * ae_factor(ap) // dp["sf"]
    assert lr == int(up["lq_size"]) and lr * dp["sf"] % ae_factor(ap) == 0, (tag, lr)   # the reference's own size rule (models/unet.py:689-702)
    return synth.synthetic_inputs(SEED_X + 1, 2, lr, lr, int(ap["embed_dim"]), hz, hz, dp["steps"], with_mask=with_mask)


def keys_of(module):
    return json.dumps([[k, list(v.shape)] for k, v in module.state_dict().items()])


def main():
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    U, V, create = ref_import.load()
    out = {}
    for tag, up in S["unet"].items():
        print(f"[unet {tag}]")
        usd = unet_weights(up)
        um = U(**up).eval()
        um.load_state_dict(usd, strict=True)
        x, t, kw = unet_inputs(tag)
        ref = um(x, t, **kw)
        check(f"unet/{tag}", oc.unet_forward(usd, up, x, t, **kw), ref, 2e-5)
        out[f"unet/{tag}"] = ref.numpy()
        out[f"keys/unet/{tag}"] = np.array(keys_of(um))
    for tag, ap in S["ae"].items():
        print(f"[ae {tag}]")
        asd = ae_weights(ap)
        am = V(**ap).eval()
        am.load_state_dict(asd, strict=True)
        img, z = ae_inputs(tag)
        ref_z = am.encode(img)
        assert ref_z.shape == z.shape
        check(f"ae/{tag}/encode", oc.vq_encode(asd, ap, img), ref_z, 2e-5)
        ref_d = am.decode(z)
        o_d, o_idx = oc.vq_decode(asd, ap, z, return_indices=True)
        check(f"ae/{tag}/decode", o_d, ref_d, 2e-5)
        _, _, (_, _, ref_idx) = am.quantize(z)
        assert torch.equal(o_idx, ref_idx)
        out[f"ae/{tag}/encode"] = ref_z.numpy()
        out[f"ae/{tag}/decode"] = ref_d.numpy()
        out[f"ae/{tag}/decode_idx"] = ref_idx.numpy().astype(np.int32)
        out[f"keys/ae/{tag}"] = np.array(keys_of(am))
    for tag in S["pairs"]:
        print(f"[pair {tag}]")
        up, ap, dp, with_mask = cases.structure_pair(tag)
        usd, asd = unet_weights(up), ae_weights(ap)
        um = U(**up).eval()
        um.load_state_dict(usd, strict=True)
        am = V(**ap).eval()
        am.load_state_dict(asd, strict=True)
        y, noises, mask = pair_inputs(tag)
        ref_img, ref_zf, ref_idx = ref_sample(create(**dp), um, am, y, noises, mask)
        o_img, aux = oc.sample_loop(usd, up, asd, ap, dp, y, noises, mask=mask, return_aux=True)
        check(f"pair/{tag}/sample z_final", aux["z_final"], ref_zf, 2e-5)
        assert (aux["indices"] == ref_idx).float().mean().item() == 1.0
        check(f"pair/{tag}/sample image", o_img, ref_img, 2e-5)
        big = ref_img.shape[-1] > 64
        out[f"pair/{tag}/sample"] = ref_img.numpy().astype(np.float16) if big else ref_img.numpy()
        out[f"pair/{tag}/sample_z"] = ref_zf.numpy()
        out[f"pair/{tag}/sample_idx"] = ref_idx.numpy().astype(np.int32)
    out["meta/seeds"] = np.array([SEED_W, SEED_X])
    np.savez_compressed(PATH, **out)
    size = os.path.getsize(PATH)
    print(f"wrote {PATH} ({size / 1024:.0f} KiB, {len(out)} arrays)")
    assert size < 512 * 1024


if __name__ == "__main__":
    main()

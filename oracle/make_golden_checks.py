"""Golden vectors for the tests of tests/test_oracle.py that used to need the reference tree itself: what the UNMODIFIED reference
produced for them is stored, so that they run wherever the repository is checked out (the reference tree and the oracle/_ref copy are
build-container / baseline artefacts, and the copy holds only the import closure of the modules - no configs/, no utils/).

  * `offsize/<h>x<w>`   the reference UNet (tiny case, constructed for 16 x 16) at 48 x 32, 32 x 16 and 16 x 48;
  * `live/unet`, `live/encode`   the tiny UNet forward and the VQ-f4 encoder on the tiny case's inputs;
  * `spec/<config>`     JSON: the model / diffusion / autoencoder sections of the reference's configs/<config>.yaml and the (key, shape)
                        lists of the state_dicts its UNetModelSwin / VQModelTorch build from them;
  * `tiling/<k>/...`    utils/util_image.py ImageSpliterTh on TILING_CASES[k]: tile origins, the canvas windows of every call, and sha256
                        digests of the patches it hands out and of its gather() after the deterministic per-tile results of tiling_result();
  * `respace/...`       respace.py SpacedDiffusion tables and timestep map for RESPACE_DP.

The oracle restatement is asserted against every output in the same run (bit-exact, as the live tests assert it).  Stored:
tests/golden/reference_checks.npz.

    python -m oracle.make_golden_checks          (needs the reference tree itself, not the oracle/_ref copy: oracle/ref_import.py)
"""
from __future__ import annotations

import hashlib
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import cases, ref_import, resshift_oracle as oc, synth  # noqa: E402
from oracle.make_golden import SEED_W  # noqa: E402
from resshift_amd.config import load_config, to_plain  # noqa: E402
from resshift_amd.spec import ae_param_spec, unet_param_spec  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
PATH = os.path.join(GOLD, "reference_checks.npz")
SEED_X = 123

OFFSIZE_SEED = 11
OFFSIZE_SIZES = ((48, 32), (32, 16), (16, 48))
SPEC_CONFIGS = ("realsr_swinunet_realesrgan256", "faceir_gfpgan512_lpips", "inpaint_lama256_imagenet")
# (H, W, pch_size, stride, sf, extra_bs)
TILING_CASES = ((96, 80, 64, 48, 4, 1), (130, 64, 64, 64, 2, 3), (64, 64, 64, 32, 4, 1), (200, 131, 64, 50, 1, 2))
RESPACE_DP = dict(cases.TINY_DIFFUSION, steps=12, timestep_respacing=4)
RESPACE_TABLES = ("sqrt_etas", "etas", "posterior_mean_coef1", "posterior_mean_coef2", "posterior_log_variance_clipped")


def tiny_weights():
    up, ap = cases.TINY_UNET, cases.TINY_AE
    uspec, _ = unet_param_spec(up)
    return synth.synthetic_state_dict(uspec, SEED_W, image_size=up["image_size"]), synth.synthetic_state_dict(ae_param_spec(ap), SEED_W)


def offsize_inputs():
    """(h, w, x, y) of the three off-size UNet calls (timestep 1, batch 2)"""
    g = torch.Generator().manual_seed(OFFSIZE_SEED)
    out = []
    for (h, w) in OFFSIZE_SIZES:
        x, y = torch.randn(2, 3, h, w, generator=g), torch.rand(2, 3, h, w, generator=g) * 2 - 1
        out.append((h, w, x, y))
    return out


def live_inputs():
    """(x, t, y, image) of the tiny case: one UNet forward and one encoder call on the bicubic x4 of its LQ input"""
    up, ap, dp = cases.TINY_UNET, cases.TINY_AE, cases.TINY_DIFFUSION
    hz = up["image_size"]
    y, noises, _ = synth.synthetic_inputs(SEED_X, 2, hz * 4 // dp["sf"], hz * 4 // dp["sf"], ap["embed_dim"], hz, hz, dp["steps"])
    return noises[1] * 1.3, torch.tensor([3, 3]), y, torch.nn.functional.interpolate(y, scale_factor=4, mode="bicubic")


def tiling_image(k):
    """platform-independent input of TILING_CASES[k]: uniform PCG64 draws (torch.randn's bits depend on the host's vector ISA)"""
    H, W = TILING_CASES[k][:2]
    return torch.from_numpy(np.random.Generator(np.random.PCG64(k)).random((2, 3, H, W), dtype=np.float32) * 2 - 1)


def tiling_result(pch, sf):
    """the deterministic per-tile "result" both accumulators are fed"""
    return torch.nn.functional.interpolate(pch, scale_factor=sf, mode="nearest") * 1.5 + 0.25


def digest(t) -> str:
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def _reference_spliter():
    """the reference tiler cannot be imported (utils/util_image.py pulls cv2 / skimage): its class source is exec'd as is"""
    src = open(os.path.join(ref_import.REF, "utils", "util_image.py")).read()
    m = re.search(r"^class ImageSpliterTh:.*?(?=^class |\Z)", src, re.S | re.M)
    ns = {"torch": torch}
    exec(m.group(0), ns)
    return ns["ImageSpliterTh"]


def main():
    torch.set_grad_enabled(False)
    U, V, create = ref_import.load()
    assert not ref_import.is_copy(), "needs the reference tree (configs/ and utils/ are not in the oracle/_ref copy)"
    out = {}
    up, ap, dp = cases.TINY_UNET, cases.TINY_AE, cases.TINY_DIFFUSION
    usd, asd = tiny_weights()
    um = U(**up).eval()
    um.load_state_dict(usd, strict=True)
    am = V(**ap).eval()
    am.load_state_dict(asd, strict=True)

    for (h, w, x, y) in offsize_inputs():
        r = um(x, torch.tensor([1, 1]), lq=y)
        assert torch.equal(oc.unet_forward(usd, up, x, torch.tensor([1, 1]), lq=y), r), (h, w)
        out[f"offsize/{h}x{w}"] = r.numpy()

    x, t, y, img = live_inputs()
    r = um(x, t, lq=y)
    assert torch.equal(oc.unet_forward(usd, up, x, t, lq=y), r)
    out["live/unet"] = r.numpy()
    z = am.encode(img)
    assert (oc.vq_encode(asd, ap, img) - z).abs().max().item() <= 2e-5 * z.abs().max().item()
    out["live/encode"] = z.numpy()

    for cname in SPEC_CONFIGS:
        ref_cfg = to_plain(load_config(os.path.join(ref_import.REF, "configs", cname + ".yaml")))
        m = U(**ref_cfg["model"]["params"])
        a = V(**ref_cfg["autoencoder"]["params"])
        rec = {"config": {sec: ref_cfg[sec] for sec in ("model", "diffusion", "autoencoder")},
               "unet": [[k, list(v.shape)] for k, v in m.state_dict().items()],
               "ae": [[k, list(v.shape)] for k, v in a.state_dict().items()]}
        out[f"spec/{cname}"] = np.array(json.dumps(rec))

    Ref = _reference_spliter()
    for k, (H, W, ps, st, sf, ebs) in enumerate(TILING_CASES):
        im = tiling_image(k)
        r = Ref(im, ps, st, sf=sf, extra_bs=ebs)
        assert r.height_starts_list == oc.tile_starts(H, ps, st) and r.width_starts_list == oc.tile_starts(W, ps, st)
        windows, pch_hash = [], hashlib.sha256()
        for pch, infos in r:
            pch_hash.update(pch.contiguous().numpy().tobytes())
            windows.append([list(i) for i in infos])
            r.update(tiling_result(pch, sf), infos)
        out[f"tiling/{k}/height_starts"] = np.array(r.height_starts_list, dtype=np.int64)
        out[f"tiling/{k}/width_starts"] = np.array(r.width_starts_list, dtype=np.int64)
        out[f"tiling/{k}/windows"] = np.array(json.dumps(windows))
        out[f"tiling/{k}/pch_sha256"] = np.array(pch_hash.hexdigest())
        out[f"tiling/{k}/gather_sha256"] = np.array(digest(r.gather()))

    ref = create(**RESPACE_DP)
    s = oc.Schedule(RESPACE_DP)
    assert list(ref.timestep_map) == s.timestep_map
    out["respace/timestep_map"] = np.array(list(ref.timestep_map), dtype=np.int64)
    for name in RESPACE_TABLES:
        r = np.asarray(getattr(ref, name), dtype=np.float64)
        assert np.array_equal(r, np.asarray(getattr(s, name), dtype=np.float64)), name
        out[f"respace/{name}"] = r

    np.savez_compressed(PATH, **out)
    print(f"[make_golden_checks] {len(out)} arrays -> {os.path.relpath(PATH, ROOT)} ({os.path.getsize(PATH) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()

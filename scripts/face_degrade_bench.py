"""The face recipe's operators: device-event times at 256 x 256 and 512 x 512, batch 32 (C = 3, seeded device tensors in
[0, 1]), by scripts/degrade_bench.py's method - the legs of an operator alternate in one process, a warm-up round, then `--rounds` rounds
of back-to-back calls between two device events; each figure is the median round, `spread` is (max - min) / median.

  jpeg_codec        rs_jpeg_codec against what a host does today - round to uint8 on the device, copy to the host, Pillow's libjpeg
                    save(quality, subsampling=2) + open per image, copy back, / 255 (the PCIe round trip is part of the leg) - and beside
                    rs_jpeg (DiffJPEG, another function).  Before timing, the codec's bytes are compared with Pillow's: `bytes_differ`.
  blur_resize_r<R>  rs_blur_resize with one 41-tap kernel per image at the ratios 1 ... 32 against F.conv2d (groups = B * C) on a
                    reflect-padded tensor + F.interpolate(bilinear) in torch.  `--blur-only`: these legs alone, without torch's - for
                    two builds of the library with another switch between the LDS-staged and the per-sample kernel
                    (RS_BUILD_DEFS=BR_SWITCH_STEP=..., RS_BUILD_OUT, RESSHIFT_HIP_LIB), which is how DESIGN.md 7i's crossing was found.
  upsample_r<R>     rs_blur_resize without a kernel, back to the full size, against F.interpolate.
  run_face          Degrader.run_face for one plan (B = 1) against the same stages composed of torch and Pillow.

`hbm_fraction`: the algorithmic bytes (input read + output written) over the call time, over the 8.0 TB/s HBM3E peak.  Prints ONE JSON line,
writes it to profiles/face_degrade_bench.json (`--out`) and makes sure profiles/INDEX.md has the file's line.

    python scripts/face_degrade_bench.py [--rounds 5] [--window 0.1]
"""
from __future__ import annotations

import argparse
import io
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from _timing import measure  # noqa: E402
from degrade_bench import BATCH, HBM_PEAK, MEASURE, SIZES, torch_filter2d  # noqa: E402
from resshift_amd import _lib, degrade  # noqa: E402

RATIOS = (1.0, 2.0, 4.0, 6.0, 8.0, 16.0, 32.0)
INDEX_LINE = ("| `face_degrade_bench.json` | `scripts/face_degrade_bench.py` (DESIGN §7i): device-event times of `rs_jpeg_codec` against Pillow on the host with "
              "the PCIe round trip and beside `rs_jpeg`, of `rs_blur_resize` (41 taps) at ratios 1 … 32 against `F.conv2d` + `F.interpolate`, and of one "
              "`run_face` plan - 256² and 512², batch 32 - median of alternating rounds, spread, fraction of the HBM peak on the algorithmic bytes |")


def pillow_roundtrip_batch(x, quality):
    """what a host does today: uint8 on the device, to the host, libjpeg per image, back, / 255"""
    from PIL import Image

    u8 = (x.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().cpu().numpy()
    out = np.empty_like(u8)
    for i, q in enumerate(quality):
        buf = io.BytesIO()
        Image.fromarray(u8[i]).save(buf, format="JPEG", quality=int(q), subsampling=2)
        buf.seek(0)
        out[i] = np.asarray(Image.open(buf).convert("RGB"))
    return torch.from_numpy(out).to(x.device).permute(0, 3, 1, 2).float() / 255


def host_face(x, plan, kernel):
    """run_face's stages composed of torch and Pillow (noise from torch.randn_like)"""
    y = F.interpolate(torch_filter2d(x, kernel), size=plan.small, mode="bilinear", align_corners=False)
    y = (y + plan.nf / 255 * torch.randn_like(y)).clamp(0, 1)
    y = pillow_roundtrip_batch(y, [plan.quality])
    y = F.interpolate(y, size=(plan.H, plan.W), mode="bilinear", align_corners=False)
    return (y * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.1, help="seconds of back-to-back calls per leg and round")
    ap.add_argument("--blur-only", action="store_true", help="only the rs_blur_resize legs, without the torch legs (A/B of two library builds)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "face_degrade_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("face_degrade_bench.py measures on the GPU: no device is visible (there is no CPU fallback)")
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    _lib.load()
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_s": args.window, "hbm_peak_bytes_per_s": HBM_PEAK, "batch": BATCH,
              "sizes": {}}
    for S in SIZES:
        g = torch.Generator().manual_seed(7)
        x = torch.rand(BATCH, 3, S, S, generator=g).to(dev)
        rng = np.random.default_rng(S)
        k41 = torch.from_numpy(np.stack([degrade.blur_kernel("aniso", 41, float(rng.uniform(4, 16)), float(rng.uniform(4, 16)), float(rng.uniform(0, np.pi)))
                                         for _ in range(BATCH)])).to(dev)
        qual = [int(q) for q in rng.integers(30, 70, BATCH)]
        ops = {}
        as_u8 = lambda t: (t * 255).round().to(torch.uint8)    # (torch divides by a scalar through its reciprocal: compare bytes, not floats)
        differ = int((as_u8(_lib.jpeg_codec(x, qual)) != as_u8(pillow_roundtrip_batch(x, qual))).sum().item())
        ops["jpeg_codec"] = ({"hip": lambda: _lib.jpeg_codec(x, qual), "pillow_host": lambda: pillow_roundtrip_batch(x, qual),
                              "rs_jpeg": lambda: _lib.jpeg(x, [float(q) for q in qual])}, "pillow_host", 2 * 4 * x.numel(), {"bytes_differ": differ})
        for r in RATIOS:
            size = (int(S // r), int(S // r))
            hip = lambda size=size: _lib.blur_resize(x, k41, size)
            ref = lambda size=size: F.interpolate(torch_filter2d(x, k41), size=size, mode="bilinear", align_corners=False)
            agree = float((hip() - ref()).abs().max().item())
            ops[f"blur_resize_r{r:g}"] = ({"hip": hip, "torch": ref}, "torch", 4 * (x.numel() + BATCH * 3 * size[0] * size[1]),
                                          {"out_size": size, "max_abs_hip_minus_torch": agree})
        for r in (4.0, 32.0):
            small = torch.rand(BATCH, 3, int(S // r), int(S // r), generator=g).to(dev)
            hip = lambda small=small: _lib.blur_resize(small, None, (S, S))
            ref = lambda small=small: F.interpolate(small, size=(S, S), mode="bilinear", align_corners=False)
            ops[f"upsample_r{r:g}"] = ({"hip": hip, "torch": ref}, "torch", 4 * (small.numel() + x.numel()),
                                       {"max_abs_hip_minus_torch": float((hip() - ref()).abs().max().item())})
        plan = degrade.face_plan(S, S, sf=8.0, sig_x=6.0, sig_y=11.0, theta=0.9, nf=10.0, qf=50.0, noise_seed=5)
        dg = degrade.Degrader(dev)
        kern = torch.from_numpy(plan.kernel()[None]).to(dev)
        ops["run_face"] = ({"hip": lambda: dg.run_face(x[:1], plan), "torch_and_pillow_host": lambda: host_face(x[:1], plan, kern)}, "torch_and_pillow_host",
                           None, {"plan": plan.to_dict()})
        rows = {}
        for name, (legs, against, traffic, extra) in ops.items():
            if args.blur_only:
                if not name.startswith("blur_resize"):
                    continue
                legs, against = {"hip": legs["hip"]}, "hip"
            res = measure(legs, args.rounds, args.window, **MEASURE)
            row = {"legs": res, "against": against, "speedup": res[against]["ms"] / res["hip"]["ms"],
                   "beats_it": res[against]["ms"] > res["hip"]["ms"] * (1 + res["hip"]["spread"]), **extra}
            if traffic is not None:
                row["algorithmic_bytes"] = int(traffic)
                row["hbm_fraction"] = row["algorithmic_bytes"] / (res["hip"]["ms"] * 1e-3) / HBM_PEAK
            rows[name] = row
        result["sizes"][str(S)] = {"operators": rows}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    index = os.path.join(os.path.dirname(os.path.abspath(args.out)), "INDEX.md")
    if os.path.exists(index) and not args.blur_only:
        text = open(index).read()
        if "`face_degrade_bench.json`" not in text:
            head, sep, rest = text.partition("|---|---|\n")
            with open(index, "w") as fh:
                fh.write(head + sep + INDEX_LINE + "\n" + rest)


if __name__ == "__main__":
    main()

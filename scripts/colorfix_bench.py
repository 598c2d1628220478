"""Colour correction: device-event times of rs_color_fix, wavelet and adain, against the torch composition of the same
definition on the same GPU, for two workloads of seeded device tensors:

  (a) tiled_photo:  B = 1, C = 3, 256 x 256 -> 1024 x 1024 (one tiled photo);
  (b) bench_batch:  B = 32, C = 3, 64 x 64 -> 256 x 256 (the benchmark's batch).

The torch composition is F.interpolate(mode="bicubic", align_corners=False), five depthwise dilated F.conv2d on F.pad(mode="replicate")
resp. torch.var / mean and the affine - what a host without the kernel would run.  The four (mode, implementation) legs of a workload
alternate in one process: one warm-up round that runs every leg, then `--rounds` rounds; a leg's round is `iters` back-to-back calls between
two device events (iters chosen per leg in the warm-up so that a window lasts about `--window` seconds; output and workspace are allocated
outside the window).  Each figure is the median round; `spread` is (max - min) / median of that leg's rounds.  `hbm_fraction` is the
algorithmic bytes (sr read + out written + lq read) over the call time, over the 8.0 TB/s HBM3E peak.  Before timing, the two
implementations are compared on the timed inputs.  Prints ONE JSON line and writes it to profiles/colorfix_bench.json (`--out`).

    python scripts/colorfix_bench.py [--rounds 7] [--window 0.2]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _timing import measure  # noqa: E402
from resshift_amd import _lib  # noqa: E402

HBM_PEAK = 8.0e12   # bytes/s, HBM3E specification of the MI355X
WORKLOADS = {"tiled_photo": (1, 3, 256, 256, 4), "bench_batch": (32, 3, 64, 64, 4)}
DILATIONS = (1, 2, 4, 8, 16)


def torch_wavelet(sr, lq, sf, kernel):
    d = sr - (F.interpolate(lq, scale_factor=sf, mode="bicubic", align_corners=False) if sf > 1 else lq)
    for dil in DILATIONS:
        d = F.conv2d(F.pad(d, (dil, dil, dil, dil), mode="replicate"), kernel, groups=sr.shape[1], dilation=dil)
    return (sr - d).clamp_(-1, 1)


def torch_adain(sr, lq):
    v_sr, m_sr = torch.var_mean(sr, dim=(2, 3), keepdim=True)
    v_lq, m_lq = torch.var_mean(lq, dim=(2, 3), keepdim=True)
    gain = ((v_lq + 1e-5) / (v_sr + 1e-5)).sqrt()
    return torch.addcmul(m_lq - m_sr * gain, sr, gain).clamp_(-1, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back calls per leg and round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colorfix_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("colorfix_bench.py measures on the GPU: no device is visible (there is no CPU fallback)")
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    lib = _lib.load()
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_s": args.window, "hbm_peak_bytes_per_s": HBM_PEAK,
              "workloads": {}}
    for name, (B, Cc, Hh, W, sf) in WORKLOADS.items():
        g = torch.Generator().manual_seed(7)
        lq = (torch.rand(B, Cc, Hh, W, generator=g) * 2 - 1).to(dev)
        sr = (0.8 * lq.repeat_interleave(sf, 2).repeat_interleave(sf, 3) + 0.3 * torch.randn(B, Cc, Hh * sf, W * sf, generator=g).to(dev) + 0.15).clamp_(-1, 1)
        out = torch.empty_like(sr)
        k1 = torch.tensor([0.25, 0.5, 0.25], device=dev)
        kernel = torch.outer(k1, k1)[None, None].repeat(Cc, 1, 1, 1).contiguous()
        st = _lib.current_stream_ptr()
        legs = {}
        for mode, m in _lib.COLOR_FIX_MODES.items():
            need = int(lib.rs_color_fix_work_bytes(B, Cc, Hh, W, sf, m))
            work = torch.empty(max(need, 4), device=dev, dtype=torch.uint8)

            def hip(m=m, work=work, need=need):
                _lib.check(lib.rs_color_fix(sr.data_ptr(), lq.data_ptr(), out.data_ptr(), B, Cc, Hh, W, sf, m, work.data_ptr(), need, st), "rs_color_fix")

            legs[(mode, "hip")] = hip
        legs[("wavelet", "torch")] = lambda: torch_wavelet(sr, lq, sf, kernel)
        legs[("adain", "torch")] = lambda: torch_adain(sr, lq)
        # the two implementations on the timed inputs
        agree = {}
        for mode in _lib.COLOR_FIX_MODES:
            legs[(mode, "hip")]()
            agree[mode] = float((out - legs[(mode, "torch")]()).abs().max().item())
        res = measure(legs, args.rounds, args.window)
        nbytes = 4 * (2 * sr.numel() + lq.numel())
        wl = {"shape": {"B": B, "C": Cc, "H": Hh, "W": W, "sf": sf}, "algorithmic_bytes": nbytes, "max_abs_hip_minus_torch": agree, "modes": {}}
        for mode in _lib.COLOR_FIX_MODES:
            row = {}
            for impl in ("hip", "torch"):
                med = res[(mode, impl)]["ms"]
                row[impl] = {**res[(mode, impl)], "bytes_per_s": nbytes / (med * 1e-3), "hbm_fraction": nbytes / (med * 1e-3) / HBM_PEAK}
            row["speedup"] = row["torch"]["ms"] / row["hip"]["ms"]
            wl["modes"][mode] = row
        result["workloads"][name] = wl
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()

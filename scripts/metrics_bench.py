"""Image metrics: times of Engine.metrics' library call against two comparators, for two workloads of seeded uint8
images [B,H,W,3] scored on the Y channel with border 0:

  (a) batch:  B = 32, 256 x 256    (the benchmark's batch of results);
  (b) photo:  B = 1,  2048 x 2048  (one tiled photo).

Legs on the GPU, device-event times: `hip` - `_lib.metrics`, the whole call (workspace and outputs allocated, two launches, the PSNR
formula); `hip_raw` - rs_metrics alone on buffers allocated beforehand; `torch_conv` - the same function composed of torch ops on the
same GPU: integer Y, then the five moments through two F.conv2d passes in float64, the map and its mean; `torch_shift` - the same with
each pass written as eleven shifted multiply-adds instead of F.conv2d (what a float64 convolution costs without a library kernel).  The
legs of a workload alternate in one process: one warm-up round that runs every leg, then `--rounds` rounds; a leg's round is `iters`
back-to-back calls between two device events (iters chosen per leg in the warm-up so that a window lasts about `--window` seconds).  Each
figure is the median round; `spread` is (max - min) / median of that leg's rounds.  `numpy_cpu` is the float64 numpy restatement
(tests/_metrics_ref.batch) on the host, wall time, best of `--cpu-runs`; it is what the reference's own functions cost per image, without
the PNG round trip.  Before timing, the legs are compared on the timed inputs.  No speed-up is promised: the figures are what they are.

Prints ONE JSON line and writes it to profiles/metrics_bench.json (`--out`).

    python scripts/metrics_bench.py [--rounds 7] [--window 0.2] [--cpu-runs 2]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _metrics_ref as M  # noqa: E402
from _timing import measure  # noqa: E402
from resshift_amd import _lib  # noqa: E402

WORKLOADS = {"batch": (32, 256, 256), "photo": (1, 2048, 2048)}


def torch_y(t):
    """uint8 [B,H,W,3] -> float64 [B,1,H,W]: the integer Y of the definition in torch ops"""
    n = t[..., 0].to(torch.int64) * M.Y_COEF[0] + t[..., 1].to(torch.int64) * M.Y_COEF[1] + t[..., 2].to(torch.int64) * M.Y_COEF[2]
    q = torch.div(n, M.Y_DEN, rounding_mode="floor")
    twice = 2 * (n - q * M.Y_DEN)
    q = q + ((twice > M.Y_DEN) | ((twice == M.Y_DEN) & (q % 2 == 1))).to(torch.int64)
    return (16 + q).to(torch.float64).unsqueeze(1)


def torch_metrics(a, b, g, conv):
    """(sse, psnr, ssim) [B] of uint8 [B,H,W,3] batches on the Y channel, border 0, in float64 torch ops"""
    x, z = torch_y(a), torch_y(b)
    B, _, Hh, W = x.shape
    sse = ((x - z) ** 2).sum((1, 2, 3))
    m = torch.cat([x, z, x * x, z * z, x * z], 1).view(B * 5, 1, Hh, W)
    if conv:
        m = F.conv2d(F.conv2d(m, g.view(1, 1, 1, 11)), g.view(1, 1, 11, 1))
    else:
        m = sum(g[k] * m[..., k:k + W - 10] for k in range(11))
        m = sum(g[k] * m[..., k:k + Hh - 10, :] for k in range(11))
    m = m.view(B, 5, Hh - 10, W - 10)
    mu1, mu2 = m[:, 0], m[:, 1]
    s1, s2, s12 = m[:, 2] - mu1 * mu1, m[:, 3] - mu2 * mu2, m[:, 4] - mu1 * mu2
    ssim = (((2 * mu1 * mu2 + M.C1) * (2 * s12 + M.C2)) / ((mu1 * mu1 + mu2 * mu2 + M.C1) * (s1 + s2 + M.C2))).mean((1, 2))
    return sse, 20.0 * torch.log10(255.0 / torch.sqrt(sse / (Hh * W))), ssim


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back calls per leg and round")
    ap.add_argument("--cpu-runs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench.py measures on the GPU: no device is visible (there is no CPU fallback)")
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    lib = _lib.load()
    g = torch.from_numpy(M.window()).to(dev)
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_s": args.window, "workloads": {}}
    for name, (B, Hh, W) in WORKLOADS.items():
        rng = np.random.default_rng(11)
        a_np = rng.integers(0, 256, (B, Hh, W, 3), dtype=np.uint8)
        b_np = np.clip(a_np.astype(np.int16) + rng.integers(-12, 13, a_np.shape), 0, 255).astype(np.uint8)
        a, b = torch.from_numpy(a_np).to(dev), torch.from_numpy(b_np).to(dev)
        need = int(lib.rs_metrics_work_bytes(B, 3, Hh, W, 0, 1))
        work = torch.empty(need // 8, device=dev, dtype=torch.int64)
        sse = torch.empty(B, device=dev, dtype=torch.int64)
        ssim = torch.empty(B, device=dev, dtype=torch.float64)
        st = _lib.current_stream_ptr()

        def raw():
            _lib.check(lib.rs_metrics(a.data_ptr(), b.data_ptr(), 0, 0, B, 3, Hh, W, 0, 1, sse.data_ptr(), ssim.data_ptr(), work.data_ptr(), need, st),
                       "rs_metrics")

        legs = {"hip": lambda: _lib.metrics(a, b), "hip_raw": raw, "torch_shift": lambda: torch_metrics(a, b, g, False)}
        conv_error = None
        try:
            torch_metrics(a, b, g, True)
            torch.cuda.synchronize()
            legs["torch_conv"] = lambda: torch_metrics(a, b, g, True)
        except RuntimeError as e:   # (a build without a float64 convolution on the device)
            conv_error = str(e).splitlines()[0][:200]
        got = _lib.metrics(a, b)
        agree = {}
        for key in ("torch_shift", "torch_conv"):
            if key in legs:
                t_sse, t_psnr, t_ssim = legs[key]()
                agree[key] = {"sse_equal": bool(torch.equal(t_sse.to(torch.int64), got["sse"])),
                              "max_abs_ssim": float((t_ssim - got["ssim"]).abs().max().item()),
                              "max_abs_psnr": float((t_psnr - got["psnr"]).abs().max().item())}
        raw()
        torch.cuda.synchronize()
        agree["hip_raw_same_bits"] = bool(torch.equal(sse, got["sse"]) and torch.equal(ssim, got["ssim"]))
        res = measure(legs, args.rounds, args.window, warm=(2, 5), min_iters=5)
        cpu = []
        for _ in range(args.cpu_runs):
            t0 = time.perf_counter()
            c_sse, c_psnr, c_ssim = M.batch(a_np, b_np, 0, True)
            cpu.append((time.perf_counter() - t0) * 1e3)
        agree["numpy_cpu"] = {"sse_equal": bool(np.array_equal(c_sse, got["sse"].cpu().numpy())),
                              "max_abs_ssim": float(np.abs(c_ssim - got["ssim"].cpu().numpy()).max()),
                              "max_abs_psnr": float(np.abs(c_psnr - got["psnr"].cpu().numpy()).max())}
        hip = res["hip"]["ms"]
        result["workloads"][name] = {
            "shape": {"B": B, "H": Hh, "W": W, "C": 3, "ycbcr": True, "border": 0}, "legs": res, "numpy_cpu_ms": min(cpu), "numpy_cpu_runs_ms": cpu,
            "agreement": agree, "torch_conv_error": conv_error,
            "ratios_over_hip": dict({k: res[k]["ms"] / hip for k in res if k != "hip"}, numpy_cpu=min(cpu) / hip)}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()

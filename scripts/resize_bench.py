"""Antialiased resize: device-event times of rs_resize against two comparators on the same GPU, for three workloads of
seeded device tensors (C = 3):

  (a) photo_half:    B = 1,  1024 x 1024 -> 512 x 512    ("x2 from the x4 model" of one tiled photo);
  (b) batch_half:    B = 32, 256 x 256   -> 128 x 128    (the benchmark's batch);
  (c) photo_x1.5:    B = 1,  1024 x 1024 -> 1536 x 1536  (an upscale).

Comparators: `dense` - the composition Mh @ x @ Mw^T with the two weight matrices of the definition (tests/_resize_ref.axis_matrix, built
beforehand, not timed): the same function, what a host without the kernel would run; `interpolate` - F.interpolate(mode="bicubic",
antialias=True), for time only: its borders differ from the definition.  The legs of a workload alternate in one process: one warm-up
round that runs every leg, then `--rounds` rounds; a leg's round is `iters` back-to-back calls between two device events (iters chosen per
leg in the warm-up so that a window lasts about `--window` seconds; rs_resize writes into an output allocated outside the window).  Each
figure is the median round; `spread` is (max - min) / median of that leg's rounds.  `hbm_fraction` is the algorithmic bytes (input read +
output written) over the call time, over the 8.0 TB/s HBM3E peak.  Before timing, rs_resize and `dense` are compared on the timed inputs.

`lds_stride`: the horizontal pass reads its LDS image at a lane stride of 1/s dwords.  rs_resize with the padded image (column x at
x + x / 32, the default) against the linear one (RS_RESIZE_LDS=linear; same bits) on B = 1, 1024 x 1024 at s = 1/2, 1/4 and 1/8, the
two legs alternating like the others.

Prints ONE JSON line, writes it to profiles/resize_bench.json (`--out`) and makes sure profiles/INDEX.md has the file's line.

    python scripts/resize_bench.py [--rounds 7] [--window 0.2]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _resize_ref as R  # noqa: E402
from _timing import measure  # noqa: E402
from resshift_amd import _lib  # noqa: E402

HBM_PEAK = 8.0e12   # bytes/s, HBM3E specification of the MI355X
WORKLOADS = {"photo_half": (1, 3, 1024, 1024, 512, 512), "batch_half": (32, 3, 256, 256, 128, 128), "photo_x1.5": (1, 3, 1024, 1024, 1536, 1536)}
LDS_SCALES = (0.5, 0.25, 0.125)
INDEX_LINE = ("| `resize_bench.json` | `scripts/resize_bench.py` (DESIGN §7f): device-event times of `rs_resize` against the dense composition "
              "`Mh @ x @ Mwᵀ` and `F.interpolate(bicubic, antialias=True)` on the same GPU - 1024² → 512² (B = 1), 256² → 128² (B = 32), 1024² → 1536² "
              "(B = 1) - median of alternating rounds, spread, fraction of the HBM peak on the algorithmic bytes; `lds_stride`: the padded against "
              "the linear LDS image at s = 1/2, 1/4, 1/8 |")


def hip_leg(lib, x, out, sh, sw, layout=None):
    B, Cc, Hh, W = x.shape
    Ho, Wo = out.shape[2:]
    st = _lib.current_stream_ptr()

    def run():
        if layout:   # (both legs of the LDS comparison set the variable, so that they carry the same host work)
            os.environ["RS_RESIZE_LDS"] = layout
        rc = lib.rs_resize(x.data_ptr(), out.data_ptr(), B, Cc, Hh, W, Ho, Wo, sh, sw, 0, st)
        if layout:
            del os.environ["RS_RESIZE_LDS"]
        _lib.check(rc, "rs_resize")

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back calls per leg and round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resize_bench.py measures on the GPU: no device is visible (there is no CPU fallback)")
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    lib = _lib.load()
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_s": args.window, "hbm_peak_bytes_per_s": HBM_PEAK,
              "workloads": {}, "lds_stride": {}}
    for name, (B, Cc, Hh, W, Ho, Wo) in WORKLOADS.items():
        g = torch.Generator().manual_seed(7)
        x = (torch.rand(B, Cc, Hh, W, generator=g) * 2 - 1).to(dev)
        out = torch.empty(B, Cc, Ho, Wo, device=dev)
        sh, sw = Ho / Hh, Wo / W
        mh = torch.from_numpy(R.axis_matrix(Hh, Ho, sh)).float().to(dev).contiguous()
        mwt = torch.from_numpy(R.axis_matrix(W, Wo, sw)).float().t().contiguous().to(dev)
        legs = {"hip": hip_leg(lib, x, out, sh, sw),
                "dense": lambda: torch.matmul(torch.matmul(mh, x), mwt),
                "interpolate": lambda: F.interpolate(x, size=(Ho, Wo), mode="bicubic", antialias=True, align_corners=False)}
        legs["hip"]()
        agree = float((out - legs["dense"]()).abs().max().item())
        res = measure(legs, args.rounds, args.window)
        nbytes = 4 * (x.numel() + out.numel())
        for row in res.values():
            row["bytes_per_s"] = nbytes / (row["ms"] * 1e-3)
            row["hbm_fraction"] = row["bytes_per_s"] / HBM_PEAK
        hip = res["hip"]
        result["workloads"][name] = {
            "shape": {"B": B, "C": Cc, "H": Hh, "W": W, "Ho": Ho, "Wo": Wo}, "algorithmic_bytes": nbytes, "max_abs_hip_minus_dense": agree,
            "legs": res, "speedup_over_dense": res["dense"]["ms"] / hip["ms"], "speedup_over_interpolate": res["interpolate"]["ms"] / hip["ms"],
            # acceptance: faster than both comparators by more than the spread of its own rounds
            "beats_both": all(res[k]["ms"] > hip["ms"] * (1 + hip["spread"]) for k in ("dense", "interpolate"))}
    g = torch.Generator().manual_seed(7)
    x = (torch.rand(1, 3, 1024, 1024, generator=g) * 2 - 1).to(dev)
    for s in LDS_SCALES:
        Ho = Wo = int(1024 * s)
        out_p, out_l = torch.empty(1, 3, Ho, Wo, device=dev), torch.empty(1, 3, Ho, Wo, device=dev)
        legs = {"padded": hip_leg(lib, x, out_p, s, s, layout="padded"), "linear": hip_leg(lib, x, out_l, s, s, layout="linear")}
        legs["padded"]()
        legs["linear"]()
        res = measure(legs, args.rounds, args.window)
        result["lds_stride"][f"{s:g}"] = {"lane_stride_dwords": 1 / s, "same_bits": bool(torch.equal(out_p, out_l)), "legs": res,
                                          "linear_over_padded": res["linear"]["ms"] / res["padded"]["ms"]}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    index = os.path.join(os.path.dirname(os.path.abspath(args.out)), "INDEX.md")
    if os.path.exists(index):
        text = open(index).read()
        if "`resize_bench.json`" not in text:
            head, sep, rest = text.partition("|---|---|\n")
            with open(index, "w") as fh:
                fh.write(head + sep + INDEX_LINE + "\n" + rest)


if __name__ == "__main__":
    main()

"""Degradation operators: device-event times of rs_filter2d, rs_interp, rs_add_noise, rs_jpeg, rs_unit_to_u8 and of a whole
plan (resshift_amd.degrade.Degrader.run) against a torch composition of the same operators on the same GPU, at 256 x 256 and 512 x 512
ground truth, batch 32 (C = 3, seeded device tensors in [0, 1]).

The torch legs are what a host without the kernels would run: F.conv2d (groups = B * C) on a reflect-padded tensor, F.interpolate, x +
c * randn clamped, the tensordot DiffJPEG written below (the formulation of the reference's basicsr/utils/diffjpeg.py: colour matrix, 2 x 2
average pooling, block split, an 8 x 8 x 8 x 8 cosine tensor, tables, merge, pixel repetition, colour matrix) and round / clamp / permute /
uint8.  The torch noise leg draws with torch.randn_like - another generator, the same traffic.  The legs of an operator alternate in one
process: a warm-up round, then `--rounds` rounds of `iters` back-to-back calls between two device events; each figure is the median
round, `spread` is (max - min) / median.  `hbm_fraction`: the algorithmic bytes (input read + output written) over the call time, over
the 8.0 TB/s HBM3E peak.  Before timing, each kernel is compared with its torch leg on the timed input (the noise legs excepted).

Prints ONE JSON line, writes it to profiles/degrade_bench.json (`--out`) and makes sure profiles/INDEX.md has the file's line.

    python scripts/degrade_bench.py [--rounds 5] [--window 0.1]
"""
from __future__ import annotations

import argparse
import itertools
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _timing import measure  # noqa: E402
from resshift_amd import _lib, degrade  # noqa: E402

HBM_PEAK = 8.0e12   # bytes/s, HBM3E specification of the MI355X
SIZES = (256, 512)
BATCH = 32
MEASURE = {"warm": (2, 5), "min_iters": 5, "max_iters": 5000}   # this script's (and face_degrade_bench.py's) arguments of _timing.measure
INDEX_LINE = ("| `degrade_bench.json` | `scripts/degrade_bench.py` (DESIGN §7h): device-event times of `rs_filter2d`, `rs_interp`, `rs_add_noise`, `rs_jpeg`, "
              "`rs_unit_to_u8` and of a whole degradation plan against a torch composition of the same operators on the same GPU - 256² and 512² ground truth, "
              "batch 32 - median of alternating rounds, spread, fraction of the HBM peak on the algorithmic bytes |")


# ---------------------------------------------------------------------------------------------------------------- the torch composition
def torch_filter2d(x, kernels):
    B, Cc, Hh, W = x.shape
    k = kernels.shape[-1]
    xp = F.pad(x, (k // 2,) * 4, mode="reflect")
    w = kernels.expand(B, k, k) if kernels.shape[0] == 1 else kernels
    w = w.view(B, 1, k, k).repeat(1, Cc, 1, 1).view(B * Cc, 1, k, k)
    return F.conv2d(xp.reshape(1, B * Cc, Hh + k - 1, W + k - 1), w, groups=B * Cc).view(B, Cc, Hh, W)


class TorchJPEG:
    """DiffJPEG(differentiable=False) as tensor operations on the device"""

    def __init__(self, dev):
        y = np.array([[16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56], [14, 17, 22, 29, 51, 87, 80, 62],
                      [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92], [49, 64, 78, 87, 103, 121, 120, 101],
                      [72, 92, 95, 98, 112, 100, 103, 99]], dtype=np.float32).T
        c = np.full((8, 8), 99, np.float32)
        c[:4, :4] = np.array([[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]], dtype=np.float32).T
        fwd = np.zeros((8, 8, 8, 8), np.float32)
        inv = np.zeros((8, 8, 8, 8), np.float32)
        for a, b, u, v in itertools.product(range(8), repeat=4):
            fwd[a, b, u, v] = np.cos((2 * a + 1) * u * np.pi / 16) * np.cos((2 * b + 1) * v * np.pi / 16)
            inv[a, b, u, v] = np.cos((2 * u + 1) * a * np.pi / 16) * np.cos((2 * v + 1) * b * np.pi / 16)
        alpha = np.array([1 / np.sqrt(2)] + [1] * 7)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        self.y, self.c, self.fwd, self.inv = t(y), t(c), t(fwd), t(inv)
        self.scale, self.alpha = t(np.outer(alpha, alpha) * 0.25), t(np.outer(alpha, alpha))
        self.m_fwd = t(np.array([[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]], dtype=np.float32).T)
        self.m_inv = t(np.array([[1.0, 0.0, 1.402], [1, -0.344136, -0.714136], [1, 1.772, 0]], dtype=np.float32).T)
        self.shift = t(np.array([0.0, 128.0, 128.0]))

    @staticmethod
    def split(p):
        B, Hh, W = p.shape
        return p.view(B, Hh // 8, 8, W // 8, 8).permute(0, 1, 3, 2, 4).contiguous().view(B, -1, 8, 8)

    @staticmethod
    def merge(b, Hh, W):
        return b.view(b.shape[0], Hh // 8, W // 8, 8, 8).permute(0, 1, 3, 2, 4).contiguous().view(b.shape[0], Hh, W)

    def __call__(self, x, quality):
        B, _, Hh, W = x.shape
        q = torch.as_tensor(quality, dtype=torch.float32, device=x.device).expand(B)
        factor = (torch.where(q < 50, 5000.0 / q, 200.0 - q * 2) / 100.0).view(B, 1, 1, 1)
        hp, wp = (-Hh) % 16, (-W) % 16
        x = F.pad(x, (0, wp, 0, hp)) * 255
        ycc = torch.tensordot(x.permute(0, 2, 3, 1), self.m_fwd, dims=1) + self.shift
        planes = [ycc[..., 0]] + [F.avg_pool2d(ycc[..., i].unsqueeze(1), 2).squeeze(1) for i in (1, 2)]
        out = []
        for p, table in zip(planes, (self.y, self.c, self.c)):
            tab = table * factor
            coef = torch.round(self.scale * torch.tensordot(self.split(p) - 128, self.fwd, dims=2) / tab)
            out.append(self.merge(0.25 * torch.tensordot(coef * tab * self.alpha, self.inv, dims=2) + 128, p.shape[1], p.shape[2]))
        up = lambda p: p.repeat_interleave(2, 1).repeat_interleave(2, 2)
        img = torch.stack([out[0], up(out[1]), up(out[2])], dim=3) - self.shift
        rgb = torch.tensordot(img, self.m_inv, dims=1).permute(0, 3, 1, 2)
        return (rgb.clamp(0, 255) / 255)[:, :, :Hh, :W]


def torch_run(plan, x, kernels, jpeg):
    """the stages of Degrader.run as torch operations (noise from torch.randn_like)"""
    def noise(x, st):
        sig = torch.tensor(st.sigma, device=x.device, dtype=torch.float32).view(-1, 1, 1, 1) / 255
        n = torch.randn_like(x)
        g = torch.tensor(st.gray, device=x.device).view(-1, 1, 1, 1)
        return (x + sig * torch.where(g, n[:, :1], n)).clamp(0, 1)

    interp = lambda x, mode, **kw: F.interpolate(x, mode=mode, **kw, **({} if mode == "area" else {"align_corners": False}))
    x = torch_filter2d(x, kernels["first"])
    x = noise(interp(x, plan.first.mode, scale_factor=plan.first.scale), plan.first)
    x = jpeg(x, plan.jpeg1)
    size = (plan.H // plan.sf, plan.W // plan.sf)
    if plan.sinc_first:
        x = torch_filter2d(interp(x, plan.final_mode, size=size), kernels["final"]).clamp(0, 1)
        x = jpeg(x, plan.jpeg2)
    else:
        x = torch_filter2d(interp(jpeg(x, plan.jpeg2), plan.final_mode, size=size), kernels["final"])
    return (x * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.1, help="seconds of back-to-back calls per leg and round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "degrade_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("degrade_bench.py measures on the GPU: no device is visible (there is no CPU fallback)")
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    _lib.load()
    jpeg_t = TorchJPEG(dev)
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_s": args.window, "hbm_peak_bytes_per_s": HBM_PEAK, "batch": BATCH,
              "sizes": {}}
    for S in SIZES:
        g = torch.Generator().manual_seed(7)
        x = torch.rand(BATCH, 3, S, S, generator=g).to(dev)
        rng = np.random.default_rng(S)
        specs = [degrade.KernelSpec("aniso", 11, 13, sig_x=float(rng.uniform(0.2, 0.8)), sig_y=float(rng.uniform(0.2, 0.8)), theta=float(rng.uniform(-3, 3)))
                 for _ in range(BATCH)]
        k13 = torch.from_numpy(np.stack([s.array() for s in specs])).to(dev)
        k21 = torch.from_numpy(degrade.sinc_kernel(0.9, 21)).unsqueeze(0).to(dev)
        qual = [float(q) for q in rng.uniform(70, 95, BATCH)]
        keys, sigma, gray = [(i + 1, 0) for i in range(BATCH)], [float(v) for v in rng.uniform(1, 15, BATCH)], [bool(v) for v in rng.uniform(size=BATCH) < 0.4]
        sig_t = torch.tensor(sigma, device=dev).view(-1, 1, 1, 1) / 255
        ops = {
            "filter2d_k13_per_image": (lambda: _lib.filter2d(x, k13), lambda: torch_filter2d(x, k13), 2),
            "filter2d_k21_shared": (lambda: _lib.filter2d(x, k21), lambda: torch_filter2d(x, k21), 2),
            "interp_bicubic_0.6": (lambda: _lib.interpolate(x, scale_factor=0.6, mode="bicubic"),
                                   lambda: F.interpolate(x, scale_factor=0.6, mode="bicubic", align_corners=False), 1.36),
            "interp_bilinear_1.3": (lambda: _lib.interpolate(x, scale_factor=1.3, mode="bilinear"),
                                    lambda: F.interpolate(x, scale_factor=1.3, mode="bilinear", align_corners=False), 2.69),
            "interp_area_quarter": (lambda: _lib.interpolate(x, size=(S // 4, S // 4), mode="area"), lambda: F.interpolate(x, size=(S // 4, S // 4), mode="area"), 1.0625),
            "add_noise": (lambda: _lib.add_noise(x, keys, sigma, gray=gray), lambda: (x + sig_t * torch.randn_like(x)).clamp(0, 1), 2),
            "jpeg": (lambda: _lib.jpeg(x, qual), lambda: jpeg_t(x, qual), 2),
            "unit_to_u8": (lambda: _lib.unit_to_u8(x), lambda: (x * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous(), 1.25),
        }
        plan = degrade.draw_plan(degrade.REALESRGAN_TESTING, BATCH, S, S, 10000)
        dg = degrade.Degrader(dev)
        kern = {"first": dg._kernels(plan.first.kernels), "final": dg._kernels(plan.final_kernels)}
        ops["pipeline"] = (lambda: dg.run(x, plan), lambda: torch_run(plan, x, kern, jpeg_t), None)
        rows = {}
        for name, (hip, ref, traffic) in ops.items():
            agree = None
            if name not in ("add_noise", "pipeline"):
                agree = float((hip().float() - ref().float()).abs().max().item())
            res = measure({"hip": hip, "torch": ref}, args.rounds, args.window, **MEASURE)
            row = {"legs": res, "max_abs_hip_minus_torch": agree, "speedup_over_torch": res["torch"]["ms"] / res["hip"]["ms"],
                   "beats_torch": res["torch"]["ms"] > res["hip"]["ms"] * (1 + res["hip"]["spread"])}
            if traffic is not None:   # algorithmic bytes in units of the input tensor's
                row["algorithmic_bytes"] = int(traffic * 4 * x.numel())
                row["hbm_fraction"] = row["algorithmic_bytes"] / (res["hip"]["ms"] * 1e-3) / HBM_PEAK
            rows[name] = row
        result["sizes"][str(S)] = {"plan_stages": plan.stages(), "first_scale": plan.first.scale, "first_mode": plan.first.mode, "operators": rows}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    index = os.path.join(os.path.dirname(os.path.abspath(args.out)), "INDEX.md")
    if os.path.exists(index):
        text = open(index).read()
        if "`degrade_bench.json`" not in text:
            head, sep, rest = text.partition("|---|---|\n")
            with open(index, "w") as fh:
                fh.write(head + sep + INDEX_LINE + "\n" + rest)


if __name__ == "__main__":
    main()

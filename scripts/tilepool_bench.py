"""Tile pool on the realsr config (synthetic weights, parity policy): prints ONE JSON line with, for two seeded workloads of device tensors,

  (a) mixed_folder:  24 LR images with sizes drawn from {64x64, 96x128, 128x128, 200x152, 256x256}, chop_size 64, chop_stride 48 (the
                     reference's --chop_size 64 option: tiles of the headline shape);
  (b) large_image:   one 256x256 LR image at chop_size 128, stride 112 (what bench.py --tiled measures);

tiles/s and images/s of `TilePool` (all images submitted, then drained) against `sample_tiled` per image with chop_bs 1 and 8.  The three
modes alternate in one process (`--reps` rounds after one warm-up round that runs every shape of every mode); each figure is the median
round, `spread` is (max - min) / median of that mode's rounds.  Host clock around work that ends in a device synchronise.

  (c) data_movement: device-event time of ONE rs_tile_gather / rs_tile_scatter launch for a full pool step's tiles against the per-tile
                     launches of the per-image path they replace (rs_window_copy crops; rs_tile_accumulate calls), enqueue included.

    python scripts/tilepool_bench.py [--reps 3]

`--blend feather` measures the feathered blend instead, and prints ONE JSON line of its own: the mixed folder through
`TilePool` with the sampler's tile_blend "uniform" and "feather" alternating round by round in one process (images/s, median round and
spread as above), and the device-event time of ONE scatter launch of a full pool step's tiles, rs_tile_scatter against
rs_tile_scatter_weighted with R = (chop_size - chop_stride) * sf, measured in alternating rounds likewise.

    python scripts/tilepool_bench.py --blend feather [--reps 5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import event_ms  # noqa: E402
from resshift_amd import ResShiftSampler, _lib  # noqa: E402
from resshift_amd.config import ConfigNode, load_config, to_plain  # noqa: E402
from resshift_amd.spec import ae_param_spec, random_state_dict, unet_param_spec  # noqa: E402
from resshift_amd.tilepool import TilePool, tile_windows  # noqa: E402

SIZES = [(64, 64), (96, 128), (128, 128), (200, 152), (256, 256)]
WORKLOADS = {"mixed_folder": dict(chop_size=64, chop_stride=48, n=24), "large_image": dict(chop_size=128, chop_stride=112, n=1)}


def workload_sizes(name):
    if name == "large_image":
        return [(256, 256)]
    rng = np.random.default_rng(17)
    return [SIZES[i] for i in rng.integers(0, len(SIZES), WORKLOADS[name]["n"])]


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def blend_bench(smp, dev, plan, reps, result):
    """uniform and feather, round by round: the mixed folder through the pool, and one scatter launch of 32 tiles of 64 x 64 (sf 4)"""
    w = WORKLOADS["mixed_folder"]
    g = torch.Generator().manual_seed(3)
    ims = [(torch.rand(1, 3, h, wd, generator=g) * 2 - 1).to(dev) for h, wd in workload_sizes("mixed_folder")]
    smp.chop_size, smp.chop_stride = w["chop_size"], w["chop_stride"]
    blends = ("uniform", "feather")

    def run_pool(blend):
        smp.tile_blend = blend
        tp = TilePool(smp)
        assert tp.blend == blend
        for y in ims:
            tp.submit(y)
        return tp.drain()

    secs = {b: [] for b in blends}
    for rnd in range(reps + 1):   # round 0 warms up
        for b in blends:
            dt, _ = sync_time(lambda: run_pool(b))
            if rnd:
                secs[b].append(dt)
            print(f"[tilepool_bench] mixed_folder round {rnd} {b}: {dt:.3f} s", file=sys.stderr, flush=True)
    smp.tile_blend = "uniform"
    out = dict(plan)
    for b, v in secs.items():
        med = float(np.median(v))
        out[b] = {"seconds": [round(x, 4) for x in v], "images_s": round(plan["images"] / med, 3), "tiles_s": round(plan["tiles"] / med, 2),
                  "spread": round((max(v) - min(v)) / med, 4)}
    out["feather_over_uniform"] = round(out["feather"]["images_s"] / out["uniform"]["images_s"], 4)
    result["mixed_folder"] = out

    n, sf, P = 32, 4, 64
    ramp = ((w["chop_size"] - w["chop_stride"]) * sf,) * 2
    wins = tile_windows(256, 256, 64, 48)
    wins = (wins + wins)[:n]
    batch = torch.rand(n, 3, P * sf, P * sf, device=dev)
    acc, cnt = torch.zeros(3, 256 * sf, 256 * sf, device=dev), torch.zeros(256 * sf, 256 * sf, device=dev)
    rows = [(acc, cnt, 256, 256, *wn) for wn in wins]
    launches = {"uniform": lambda: _lib.tile_scatter(rows, batch, sf), "feather": lambda: _lib.tile_scatter(rows, batch, sf, ramp=ramp)}
    ms = {b: [] for b in blends}
    for rnd in range(reps + 1):
        for b in blends:
            t = event_ms(launches[b], 50, warm=1)
            if rnd:
                ms[b].append(t)
    result["scatter_launch"] = {"tiles_per_step": n, "tile": "64x64 LR, sf 4", "ramp": ramp[0], "iters_per_round": 50}
    for b, v in ms.items():
        med = float(np.median(v))
        result["scatter_launch"][b] = {"ms": [round(x, 4) for x in v], "median_ms": round(med, 4), "spread": round((max(v) - min(v)) / med, 4)}
    result["scatter_launch"]["feather_over_uniform"] = round(result["scatter_launch"]["feather"]["median_ms"]
                                                             / result["scatter_launch"]["uniform"]["median_ms"], 4)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--blend", choices=["feather"], default=None, help="measure the feathered blend against the uniform one instead")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    plan = {}
    for name, w in WORKLOADS.items():
        sizes = workload_sizes(name)
        tiles = [len(tile_windows(h, wd, w["chop_size"], w["chop_stride"])) for h, wd in sizes]
        plan[name] = {"images": len(sizes), "tiles": int(sum(tiles)), "chop_size": w["chop_size"], "chop_stride": w["chop_stride"],
                      "sizes": ["%dx%d" % s for s in sizes]}
        print(f"[tilepool_bench] {name}: {len(sizes)} images, {sum(tiles)} tiles", file=sys.stderr, flush=True)
    dev = torch.device("cuda:0")
    cfg = to_plain(load_config("realsr_swinunet_realesrgan256"))
    up, aep, dp = cfg["model"]["params"], cfg["autoencoder"]["params"], cfg["diffusion"]["params"]
    sds = {"model": random_state_dict(unet_param_spec(up)[0], seed=1), "autoencoder": random_state_dict(ae_param_spec(aep), seed=2)}
    conf = ConfigNode(model=ConfigNode(target="models.unet.UNetModelSwin", ckpt_path=None, params=up),
                      diffusion=ConfigNode(target="models.script_util.create_gaussian_diffusion", params=dp),
                      autoencoder=ConfigNode(target="ldm.models.autoencoder.VQModelTorch", ckpt_path=None, params=aep))
    smp = ResShiftSampler(conf, sf=4, use_amp=True, padding_offset=64, seed=7, state_dicts=sds, precision="parity")
    result = {"config": "realsr_swinunet_realesrgan256", "policy": "parity", "reps": args.reps}
    if args.blend:
        print(json.dumps(blend_bench(smp, dev, plan["mixed_folder"], args.reps, result)), flush=True)
        return

    for name, w in WORKLOADS.items():
        g = torch.Generator().manual_seed(3)
        ims = [(torch.rand(1, 3, h, wd, generator=g) * 2 - 1).to(dev) for h, wd in workload_sizes(name)]
        smp.chop_size, smp.chop_stride = w["chop_size"], w["chop_stride"]

        def run_pool():
            tp = TilePool(smp)
            for y in ims:
                tp.submit(y)
            return tp.drain()

        def run_tiled(bs):
            smp.chop_bs = bs
            return [smp.sample_tiled(y) for y in ims]

        modes = {"tile_pool": run_pool, "sample_tiled_chop_bs1": lambda: run_tiled(1), "sample_tiled_chop_bs8": lambda: run_tiled(8)}
        secs = {m: [] for m in modes}
        for rnd in range(args.reps + 1):   # round 0 warms up every shape of every mode (arena growth, first launches)
            for m, fn in modes.items():
                dt, _ = sync_time(fn)
                if rnd:
                    secs[m].append(dt)
                print(f"[tilepool_bench] {name} round {rnd} {m}: {dt:.3f} s", file=sys.stderr, flush=True)
        out = dict(plan[name])
        for m, v in secs.items():
            med = float(np.median(v))
            out[m] = {"seconds": [round(x, 4) for x in v], "tiles_s": round(plan[name]["tiles"] / med, 2),
                      "images_s": round(plan[name]["images"] / med, 3), "spread": round((max(v) - min(v)) / med, 4)}
        out["pool_over_chop_bs8"] = round(out["tile_pool"]["tiles_s"] / out["sample_tiled_chop_bs8"]["tiles_s"], 4)
        out["pool_over_chop_bs1"] = round(out["tile_pool"]["tiles_s"] / out["sample_tiled_chop_bs1"]["tiles_s"], 4)
        result[name] = out

    # (c) the data movement of one full pool step of 64x64 tiles (32 tiles of a 256x256 image, sf 4)
    n, sf, P = 32, 4, 64
    lib = _lib.load()
    src = torch.rand(3, 256, 256, device=dev)
    wins = tile_windows(256, 256, 64, 48)
    wins = (wins + wins)[:n]
    out_lq = torch.empty(n, 3, P, P, device=dev)
    crops = torch.empty(n, 3, P, P, device=dev)
    batch = torch.rand(n, 3, P * sf, P * sf, device=dev)
    acc, cnt = torch.zeros(3, 256 * sf, 256 * sf, device=dev), torch.zeros(256 * sf, 256 * sf, device=dev)
    st = _lib.current_stream_ptr()
    g_rows = [(src, *wn) for wn in wins]
    s_rows = [(acc, cnt, 256, 256, *wn) for wn in wins]

    def per_tile_crops():
        for k, (h0, w0, th, tw) in enumerate(wins):
            _lib.window_copy(src, h0, w0, th, tw, out=crops[k])

    def per_tile_accumulate():
        for k, (h0, w0, th, tw) in enumerate(wins):
            _lib.check(lib.rs_tile_accumulate(acc.data_ptr(), cnt.data_ptr(), batch[k].data_ptr(), 1, 3, 256 * sf, 256 * sf, h0 * sf, w0 * sf,
                                              th * sf, tw * sf, st), "rs_tile_accumulate")

    result["data_movement"] = {
        "tiles_per_step": n, "tile": "64x64 LR, sf 4",
        "rs_tile_gather_ms": round(event_ms(lambda: _lib.tile_gather(g_rows, out_lq), 50, warm=1), 4),
        "per_tile_window_copy_ms": round(event_ms(per_tile_crops, 50, warm=1), 4),
        "rs_tile_scatter_ms": round(event_ms(lambda: _lib.tile_scatter(s_rows, batch, sf), 50, warm=1), 4),
        "per_tile_accumulate_ms": round(event_ms(per_tile_accumulate, 50, warm=1), 4)}
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()

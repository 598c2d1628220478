"""Continuous batching on the realsr config (synthetic weights, parity policy): prints ONE JSON line with

  (a) step_ms:    rs_sample_step at B = 32 with every image at one step vs each at its own, alternated in one process (median ms);
  (b) saturated:  ContinuousSampler img/s with a full pool vs rs_sample img/s at B = 32;
  (c) staggered:  a fixed-seed arrival schedule (Poisson, 80 % of the rs_sample rate): p50 / p95 request latency and img/s of the
                  ContinuousSampler vs waiting for full batches of 32 (each batch one rs_sample call, started when its 32nd request has
                  arrived and the previous batch is done).

    python scripts/continuous_bench.py [--reps 10] [--requests 96]

`--seeded` measures instead the seeded pool (per-request Philox noise generated inside the step's kernel) against the tensor
pool in ONE process, alternated round by round: (d) the pool's step at B = 32 with mixed step indices - tensor: the per-step gather of
each slot's draw from the [B, steps+1, ...] pool tensor + rs_sample_step; seeded: rs_sample_step_seeded alone - and (e) saturated img/s
of `ContinuousSampler(seeded=...)` over 4 pool-loads.  Medians with the min / max of the rounds (the spread).  `--out FILE` also writes
the JSON to FILE.

    python scripts/continuous_bench.py --seeded [--reps 10] [--out profiles/continuous_seeded.json]
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
from resshift_amd import ResShiftSampler  # noqa: E402
from resshift_amd.config import ConfigNode, load_config, to_plain  # noqa: E402
from resshift_amd.continuous import ContinuousSampler  # noqa: E402
from resshift_amd.spec import ae_param_spec, random_state_dict, unet_param_spec  # noqa: E402

B, LR = 32, 64


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def spread(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3), "rounds": len(v)}


def seeded_vs_tensor(args, smp, y, dev):
    """(d) + (e) of the module docstring; returns the result dict"""
    d, eng = smp.base_diffusion, smp.engine
    tables, T, sf = d.step_tables(), d.num_timesteps, d.sf
    prec = d._unet_precisions()[0]
    g = torch.Generator().manual_seed(5)
    zs = eng.latent_shape(B, LR, LR, sf)
    x0 = torch.randn(zs, generator=g).to(dev)
    pool_n = torch.randn((B, T + 1) + tuple(zs[1:]), generator=g).to(dev)   # the tensor pool's _N
    keys = [(1000 + b, 0) for b in range(B)]
    ts = [b % T for b in range(B)]
    rows = torch.arange(B, device=dev)

    def tensor_step(x):
        k = torch.tensor([T - t for t in ts], device=dev, dtype=torch.long)   # as ContinuousSampler._step_batch
        eng.sample_step(x, y, ts, pool_n[rows, k], tables, sf, prec=prec)

    def seeded_step(x):
        eng.sample_step(x, y, ts, None, tables, sf, prec=prec, keys=keys)

    x = x0.clone()
    for fn in (tensor_step, seeded_step):   # (arena growth, first launches)
        fn(x)
    t_ms, s_ms = [], []
    for r in range(args.reps):
        for fn, acc in ((tensor_step, t_ms), (seeded_step, s_ms))[:: 1 if r % 2 == 0 else -1]:
            x.copy_(x0)
            acc.append(1e3 * sync_time(lambda: fn(x))[0])
    pools = {False: ContinuousSampler(smp, max_batch=B), True: ContinuousSampler(smp, max_batch=B, seeded=True)}
    for cs in pools.values():   # (pool allocation, first calls)
        cs.submit(y)
        cs.drain()
    rate = {False: [], True: []}
    for r in range(max(3, args.reps // 2)):
        for seeded in ((False, True) if r % 2 == 0 else (True, False)):
            cs = pools[seeded]

            def load():   # submit time counts: the tensor pool draws steps + 1 latents per image there
                for _ in range(4):
                    cs.submit(y)
                cs.drain()

            sec, _ = sync_time(load)
            rate[seeded].append(4 * B / sec)
    res = {"config": "realsr_swinunet_realesrgan256", "policy": "parity", "batch": B,
           "step_ms_mixed_b32": {"tensor_gather_plus_step": spread(t_ms), "seeded_step": spread(s_ms)},
           "saturated_img_s": {"tensor_pool": spread(rate[False]), "seeded_pool": spread(rate[True])}}
    res["step_ms_mixed_b32"]["seeded_over_tensor"] = round(res["step_ms_mixed_b32"]["seeded_step"]["median"] / res["step_ms_mixed_b32"]["tensor_gather_plus_step"]["median"], 4)
    res["saturated_img_s"]["seeded_over_tensor"] = round(res["saturated_img_s"]["seeded_pool"]["median"] / res["saturated_img_s"]["tensor_pool"]["median"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--requests", type=int, default=96)
    ap.add_argument("--seeded", action="store_true", help="seeded pool vs tensor pool, alternated in one process (module docstring)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    cfg = to_plain(load_config("realsr_swinunet_realesrgan256"))
    up, aep, dp = cfg["model"]["params"], cfg["autoencoder"]["params"], cfg["diffusion"]["params"]
    sds = {"model": random_state_dict(unet_param_spec(up)[0], seed=1), "autoencoder": random_state_dict(ae_param_spec(aep), seed=2)}
    conf = ConfigNode(model=ConfigNode(target="models.unet.UNetModelSwin", ckpt_path=None, params=up),
                      diffusion=ConfigNode(target="models.script_util.create_gaussian_diffusion", params=dp),
                      autoencoder=ConfigNode(target="ldm.models.autoencoder.VQModelTorch", ckpt_path=None, params=aep))
    smp = ResShiftSampler(conf, sf=4, use_amp=True, padding_offset=64, seed=7, state_dicts=sds, precision="parity")
    d, eng = smp.base_diffusion, smp.engine
    tables, T, sf = d.step_tables(), d.num_timesteps, d.sf
    prec = d._unet_precisions()[0]
    g = torch.Generator().manual_seed(5)
    y = (torch.rand(B, 3, LR, LR, generator=g) * 2 - 1).to(dev)
    eng.film_prewarm([int(v) for v in tables["tmap"]])
    if args.seeded:
        line = json.dumps(seeded_vs_tensor(args, smp, y, dev))
        print(line, flush=True)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(line + "\n")
        return
    zs = eng.latent_shape(B, LR, LR, sf)
    noise = torch.randn(zs, generator=g).to(dev)
    x0 = torch.randn(zs, generator=g).to(dev)

    # (a) one step at B = 32: homogeneous vs mixed step indices, alternated
    t_h, t_m = [T // 2] * B, [b % T for b in range(B)]
    x = x0.clone()
    for t in (t_h, t_m):   # (arena growth, first launches)
        eng.sample_step(x, y, t, noise, tables, sf, prec=prec)
    hom, mix = [], []
    for _ in range(args.reps):
        for t, acc in ((t_h, hom), (t_m, mix)):
            x.copy_(x0)
            acc.append(1e3 * sync_time(lambda: eng.sample_step(x, y, t, noise, tables, sf, prec=prec))[0])
    step = {"homogeneous_ms": round(float(np.median(hom)), 3), "mixed_ms": round(float(np.median(mix)), 3)}
    step["mixed_over_homogeneous"] = round(step["mixed_ms"] / step["homogeneous_ms"], 4)

    # (b) saturated: rs_sample at B = 32 vs a full ContinuousSampler pool (4 pool-loads of requests)
    noises = torch.randn((T + 1,) + zs, generator=g).to(dev)
    eng.sample(y, noises, tables, sf=sf, scale_factor=d.scale_factor, prec_unet=prec, prec_encode=d._prec(d.precision_encode),
               prec_decode=d._prec(d.precision_decode))
    rs = [sync_time(lambda: eng.sample(y, noises, tables, sf=sf, scale_factor=d.scale_factor, prec_unet=prec,
                                       prec_encode=d._prec(d.precision_encode), prec_decode=d._prec(d.precision_decode)))[0] for _ in range(3)]
    batch_s = float(np.median(rs))
    cs = ContinuousSampler(smp, max_batch=B)
    cs.submit(y)
    cs.drain()   # (pool allocation, first calls)
    for _ in range(4):
        cs.submit(y)
    sec, _ = sync_time(cs.drain)
    saturated = {"rs_sample_img_s": round(B / batch_s, 2), "continuous_img_s": round(4 * B / sec, 2), "rs_sample_ms_b32": round(1e3 * batch_s, 2)}

    # (c) staggered arrivals (fixed seed): continuous vs full batches of 32
    rate = 0.8 * B / batch_s   # requests per second
    arr = np.cumsum(np.random.default_rng(11).exponential(1.0 / rate, args.requests))
    y1 = y[:1]
    done, start = {}, time.perf_counter()
    nxt, arrive_of = 0, {}
    while nxt < len(arr) or cs.pending():
        now = time.perf_counter() - start
        while nxt < len(arr) and arr[nxt] <= now:
            arrive_of[cs.submit(y1)[0]] = arr[nxt]
            nxt += 1
        if not cs.pending():
            time.sleep(max(0.0, arr[nxt] - now))
            continue
        out = cs.step()
        if out:
            torch.cuda.synchronize()
            t = time.perf_counter() - start
            for rid in out:
                done[rid] = t
    lat_c = np.array([done[r] - arrive_of[r] for r in done])
    span_c = max(done.values()) - arr[0]
    # full batches of 32: batch k starts when request 32k+31 has arrived and batch k-1 is done
    free, lat_b, last = 0.0, [], 0.0
    nb = len(arr) // B
    for k in range(nb):
        st = max(free, arr[(k + 1) * B - 1])
        now = time.perf_counter() - start
        if st > now:
            time.sleep(st - now)
        dt, _ = sync_time(lambda: eng.sample(y, noises, tables, sf=sf, scale_factor=d.scale_factor, prec_unet=prec,
                                             prec_encode=d._prec(d.precision_encode), prec_decode=d._prec(d.precision_decode)))
        free = max(st, time.perf_counter() - start - dt) + dt
        lat_b += [free - a for a in arr[k * B:(k + 1) * B]]
        last = free
    lat_b = np.array(lat_b)
    stag = {"requests": int(len(arr)), "arrival_rate_per_s": round(rate, 2),
            "continuous": {"p50_ms": round(1e3 * float(np.percentile(lat_c, 50)), 1), "p95_ms": round(1e3 * float(np.percentile(lat_c, 95)), 1),
                           "img_s": round(len(lat_c) / span_c, 2)},
            "full_batches_32": {"p50_ms": round(1e3 * float(np.percentile(lat_b, 50)), 1), "p95_ms": round(1e3 * float(np.percentile(lat_b, 95)), 1),
                                "img_s": round(len(lat_b) / (last - arr[0]), 2)}}
    line = json.dumps({"config": "realsr_swinunet_realesrgan256", "policy": "parity", "batch": B, "step_ms": step, "saturated": saturated,
                       "staggered": stag})
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

"""Every autoencoder block of the production kernel graph against float64, teacher-forced, per image.

The autoencoder's kernel choice depends on batch, shape and storage: the sub-pixel form of the upsampling conv (four 2x2 convs with summed
weights, fp16 / split storage, only when the low-resolution grid has >= 16384 pixels over the batch) or the folded-address 3x3 conv, the
1x1 shortcut folded into conv2's K loop, streaming attention (fp16: T % 128 == 0, split: T % 64 == 0) or the row-block path with a
materialised softmax, GroupNorm tails and epilogue statistics, the fused head, the asymmetric-pad stride-2 conv, the 3- / 8-channel ends
padded to 8.  A traced Engine.vq_encode / vq_decode (Engine.debug_enable) runs that same graph - the test asserts it: same output bits, same
launch count - and records every block boundary.  Each block of the plan (oracle/resshift_oracle.py: ae_encode_plan / ae_decode_plan) is
then fed the engine's own recorded inputs in float64 and compared with the engine's output of that block, per image: max |engine - ref| /
max |ref| over the image's block output, for up to 8 images spread over the batch (8 * 64 * 64 latent pixels in all).  Every case also asserts, from the families of the traced
pass and the launch shapes of a profiled pass, that it ran the kernels it is there for.  Run with -s for the table of the worst error per
block and precision.

The VQ step: the engine's indices are checked against float64 distances recomputed from the recorded latents (helpers.vq_check: the float64
argmin, or within 8 * 2^-23 * (|z|^2 + max |e|^2) of it; at most 0.1 % of an image's positions may differ from the float64 argmin at all -
tests/test_ae_blocks_cpu.py shows that the fp32 CPU oracle meets this on the same latents).  dec.zq must be, bit for bit, the codebook row
of the engine's index passed through the reference's fp32 straight-through expression z + (e[idx] - z) (quantize.py:298; that expression is
within an fp32 rounding or two of the row but not always the row itself, in the reference as in the engine), and dec.pq is teacher-forced
from the engine's dec.zq, so a legitimately tied index does not propagate.

Memory: the engine's capture region, in device memory, holds every record of the whole batch - 16.0 GiB for the largest case (realsr
decode at batch 32; faceir decode at batch 16: 15.0 GiB, realsr encode at batch 32: 10.6 GiB, faceir encode at batch 16: 9.1 GiB; printed
per case).  Only the plan's blocks of the picked images are copied out of it (Engine.debug_trace(names, images)), so the host holds 8
images per block: 2.9 GiB of fp32 for that largest case."""
import numpy as np
import pytest
import torch

import _regimes as R
import helpers as H
from oracle import resshift_oracle as oc
from resshift_amd.config import load_config, to_plain
from resshift_amd.engine import Engine, parse_precision
from resshift_amd.spec import ae_param_spec

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

CONFIGS = {"realsr": "realsr_swinunet_realesrgan256", "faceir": "faceir_gfpgan512_lpips"}
# what a case is there for.  attn: the streaming kernel of that storage ("flash16" / "flash_split") or the row-block path with the
# materialised softmax ("rows"); subpixel / folded: the decoder levels whose upsampling step must run as four 2x2 launches / as one
# folded-address 3x3 conv.
#        net      call      B   H    W    prec     attn           subpixel    folded
CASES = [("realsr", "encode", 32, 256, 256, "split", "flash_split", (), ()),
         ("realsr", "encode", 32, 256, 256, "fp16", "flash16", (), ()),
         ("realsr", "encode", 32, 256, 256, "fp32", "rows", (), ()),
         ("realsr", "decode", 32, 64, 64, "fp16", "flash16", (2, 1), ()),
         ("realsr", "decode", 32, 64, 64, "split", "flash_split", (2, 1), ()),
         ("realsr", "decode", 32, 64, 64, "fp32", "rows", (), (2, 1)),
         ("realsr", "encode", 3, 256, 256, "fp16", "flash16", (), ()),
         ("realsr", "encode", 3, 256, 256, "split", "flash_split", (), ()),
         ("realsr", "decode", 3, 64, 64, "fp16", "flash16", (1,), (2,)),
         ("realsr", "decode", 3, 64, 64, "split", "flash_split", (1,), (2,)),
         ("faceir", "encode", 16, 512, 512, "split", "flash_split", (), ()),
         ("faceir", "decode", 16, 64, 64, "fp16", "flash16", (3, 2, 1), ()),
         ("realsr", "decode", 2, 40, 24, "fp16", "rows", (), (2, 1)),
         ("realsr", "decode", 2, 40, 24, "split", "flash_split", (), (2, 1)),
         ("realsr", "decode_nq", 2, 64, 64, "fp16", "flash16", (1,), (2,)),
         # what the tile pool and the default tiled path (chop_size 128, chop_bs 1) hand the autoencoder: non-square size classes, batch 1, a
         # plane larger than the constructed one.  Decode at batch 1: 64 x 128 has 8192 low-resolution pixels at level 2 (folded form) and
         # 32768 at level 1; 128 x 128 has exactly 16384 at level 2, the threshold of the sub-pixel form, and T = 16384 tokens of attention
         ("realsr", "encode", 1, 256, 512, "split", "flash_split", (), ()),
         ("realsr", "decode", 1, 64, 128, "fp16", "flash16", (1,), (2,)),
         ("realsr", "decode", 6, 128, 64, "fp16", "flash16", (2, 1), ()),
         ("realsr", "decode", 1, 128, 128, "fp16", "flash16", (2, 1), ()),
         ("realsr", "decode", 1, 64, 128, "split", "flash_split", (1,), (2,))]
# Per-image tolerance of every block, per precision: the per-block tolerances of tests/test_unet_blocks_gpu.py (the same kernel families;
# the longest reduction here is 9 x 512 products against 9 x 640 there).  For scale, on the CPU (one realsr decoder pass, every block
# teacher-forced): the fp32 oracle is within 3.4e-7 of float64 on every block, a model of fp16 storage (float64 arithmetic; weights, conv1
# output and block output rounded to fp16) within 2.1e-4 .. 4.8e-4.
# Measured on the MI355X, worst image over all CASES (the margin; it does not define the bound; the whole table is in DESIGN 4.4):
# split 3.57e-6 (enc.out, the fused head: 9 x 512 products in one fp32 sum, 3.1e-6 in fp16 and fp32 storage as well; dec.mid.block_1 1.9e-6,
# dec.head 1.6e-6, every other block <= 1.21e-6), fp16 6.85e-4 (dec.up.0.block.0; dec.mid.block_1 6.3e-4, dec.up.1.block.0 6.2e-4, every
# block 4.0e-4 .. 6.9e-4 except the fp32-output heads), fp32 3.25e-6 (the upsampling and stride-2 convs dec.up.2.us / dec.up.1.us /
# enc.down.1.ds: 3.2e-6 / 2.9e-6 / 2.9e-6, dec.mid.block_1 2.7e-6, every other block <= 2.0e-6).  VQ: at most 1 position of an image's
# 4096 (2.4e-4) differs from the float64 argmin, within the fp32-rounding slack, in split and fp16 decodes alike - the worst image of the
# fp32 CPU oracle differs in one position too.
# The tile pool's shapes (the last five CASES: non-square, batch 1, a 128 x 128 latent) keep these bounds.  Measured over them: split 3.29e-6
# (enc.out, encode 256 x 512; decode 64 x 128: 1.78e-6, dec.head), fp16 5.76e-4 (dec.up.0.block.0, B = 6 at 128 x 64; 5.4e-4 / 5.1e-4 at batch 1
# on 64 x 128 / 128 x 128).  VQ: at most 1 position of an image's 8192 (1.2e-4) differs from the float64 argmin.
TOL = {"split": 5e-6, "fp16": 2.5e-3, "fp32": 1e-5}
F_AEFLASH, F_AEFLASH_S = 9, 10   # Engine.FAMILIES
# The weight regimes (oracle/synth.py: regime_state_dict; what each exercises is pinned on the CPU, tests/test_ae_blocks_cpu.py): the cases
# above all load one draw, in which no GroupNorm variance comes within 1e5 of eps and the attention softmax is diffuse (median largest
# probability 0.006).  "quiet" (the median variance ~30 eps, the smallest 0.02 eps), "loud" (q, k weights x 4, biases x 20: logits to 50 / 90,
# median largest probability 0.7 / 0.9 - the max subtraction and the online rescale of the streaming kernels with a large jump of the running
# maximum) and "zero_init" (the autoencoder has no zero_module tensors: the synthetic draw again) run the smallest encode and the smallest
# decode case above at B = 1.  The tolerance of a block there is max(TOL[prec], k * err32): err32 is the same plan step evaluated by the
# oracle in float32 on the same teacher-forced inputs against its float64 value, per image, the same max-norm - the reference's own
# arithmetic, never the engine's (<= 1e-4 on every block: asserted on the CPU) - with k = 4 for fp32 storage (another summation order, x 2
# margin) and k = 8 for split (the pair keeps 2^-22 of an operand, 4 x fp32's unit, x 2 margin).  fp16 storage keeps TOL["fp16"]; the
# decoder runs in it for quiet and zero_init (the parity policy's decoder is fp16).  It is left out of loud: with logits of 50 .. 90 the fp16
# rounding of q and k inside the attention block moves probabilities by percents - conditioning, not a kernel property
# (tests/test_engine_gpu.py: test_fp16_error_on_natural_images_is_conditioning_not_a_kernel makes the same point).
# Measured on the MI355X (the block nearest its tolerance: error / err32; k * err32 stayed under TOL[prec] everywhere, so TOL[prec] applied):
# encode - quiet split 2.49e-6 / 4.1e-7 (enc.out), fp32 2.88e-6 / 5.7e-7 (enc.down.1.block.0); loud split 4.82e-6 / 4.8e-7, fp32 4.90e-6 /
# 5.4e-7 (enc.out both: the fused head's 9 x 512 products in one fp32 sum, in fp32 storage as well; 3.6e-6 in the base cases);
# zero_init split 2.77e-6, fp32 2.75e-6 (enc.out).  decode - quiet split 1.36e-6 / 4.3e-7 (dec.head), fp32 1.12e-6, fp16 8.59e-4
# (dec.up.0.block.0); loud split 2.47e-6 / 2.5e-7 (dec.head), fp32 2.77e-6 / 3.6e-7 (dec.up.1.us); zero_init split 1.02e-6, fp32 1.83e-6,
# fp16 6.90e-4.
#               net      call      B   H    W    prec     attn           subpixel folded  regime
REGIME_CASES = ([("realsr", "encode", 1, 256, 256, prec, {"split": "flash_split", "fp32": "rows"}[prec], (), (), regime)
                 for regime in R.REGIMES for prec in ("split", "fp32")] +
                [("realsr", "decode", 1, 40, 24, prec, {"split": "flash_split", "fp32": "rows", "fp16": "rows"}[prec], (), (2, 1), regime)
                 for regime in R.REGIMES for prec in (("split", "fp32") if regime == "loud" else ("split", "fp32", "fp16"))])
ALL_CASES = [c + ("base",) for c in CASES] + REGIME_CASES

_models = {}
_worst = {}   # (block, prec) -> worst per-image error over the base cases run so far
_worst_regime = {}   # (regime, call, prec) -> (error of the block and image nearest its tolerance, block, its err32 or NaN, tolerance applied, worst err32)


@pytest.fixture(scope="module", autouse=True)
def _table():
    """after the module: the table of the worst per-image error per block and precision over every case that ran (-s)"""
    yield
    if not _worst:
        return
    precs = [p for p in TOL if any(pp == p for _, pp in _worst)]
    names = list(dict.fromkeys(n for n, _ in _worst))
    print("\nworst per-image error per block (max |engine - float64| / max |float64|, teacher-forced):")
    print(f"{'block':<20}" + "".join(f"{p:>12}" for p in precs))
    for n in names:
        print(f"{n:<20}" + "".join(f"{_worst.get((n, p), float('nan')):>12.3e}" for p in precs))
    print(f"{'worst block':<20}" + "".join(f"{max(v for (n, pp), v in _worst.items() if pp == p and not n.startswith('dec.idx')):>12.3e}" for p in precs))
    print(f"{'tolerance':<20}" + "".join(f"{TOL[p]:>12.1e}" for p in precs))
    if _worst_regime:
        print("\nweight regimes (realsr, B = 1): the block nearest its tolerance - error, the float32 oracle's error there (err32), tolerance applied - "
              "and the worst err32 of any block:")
        for (regime, call, prec), (e, name, e32, tol, w32) in _worst_regime.items():
            print(f"{regime:<10}{call:<8}{prec:<6}{e:>12.3e} ({name}){e32:>12.3e}{tol:>12.3e}{w32:>12.3e}")
    _models.clear()


def _model(key, gpu, regime="base"):
    """one Engine per (config, regime)"""
    key, cname = (key, regime), key
    if key not in _models:
        ap = to_plain(load_config(CONFIGS[cname]))["autoencoder"]["params"]
        asd = R.regime_sd(H.synth.synthetic_state_dict(ae_param_spec(ap), H.SEED_W), regime)
        sd64 = {k: v.double() for k, v in asd.items()}
        eng = Engine(unet_params=None, ae_params=ap, device=gpu)
        eng.load_state_dicts(ae_sd=asd)
        eng.mark_weights_ready()
        _models[key] = (ap, asd, sd64, eng)
    return _models[key]


def _pick(B, h=64, w=64):
    """images spread over the batch, the first and the last included, as many as the budget of 8 * 64 * 64 latent pixels allows: 8 at a 64 x 64
    latent, 4 at 64 x 128, 2 at 128 x 128 (all of a smaller batch)"""
    return sorted(set(int(v) for v in np.linspace(0, B - 1, min(B, max(2, 8 * 64 * 64 // (h * w)))).round()))


def _launches(shapes, part, M, N, K):
    """launches of the implicit-GEMM families (not the streaming attention kernels, which are noted as T x T x C) with this shape"""
    return sum(s["launches"] for s in shapes
               if s["part"] == part and s["family"] not in (F_AEFLASH, F_AEFLASH_S) and (s["M"], s["N"], s["K"]) == (M, N, K))


def check_kernels(ap, call, B, h, w, attn, subpixel, folded, fam, shapes):
    """the case ran what it is there for: `fam` = launches per kernel family of the traced pass (Engine.profile_families), `shapes` = the
    launch shapes of the profiled pass (Engine.profile_shapes)"""
    dd = ap["ddconfig"]
    mult = [int(m) for m in dd["ch_mult"]]
    part = "encoder" if call == "encode" else "decoder"
    f = 2 ** (len(mult) - 1)
    hl, wl = (h // f, w // f) if call == "encode" else (h, w)    # the mid block's plane
    C, T = int(dd["ch"]) * mult[-1], hl * wl
    want = {"flash16": (1, 0), "flash_split": (0, 1), "rows": (0, 0)}[attn]
    assert (fam[F_AEFLASH], fam[F_AEFLASH_S]) == want, (attn, fam)
    s_gemm = _launches(shapes, part, T, T, C)
    if attn == "rows":   # Q K^T into the materialised score matrix (the softmax kernel reads it): [T, T] with K = C, once per image chunk
        assert s_gemm >= 1, shapes
    else:
        assert s_gemm == 0, shapes
    assert set(subpixel) | set(folded) == (set(range(1, len(mult))) if call != "encode" else set()), (subpixel, folded)
    for l in range(len(mult) - 1, 0, -1):
        c = int(dd["ch"]) * mult[l]
        s = 2 ** (len(mult) - 1 - l)
        m_lo = B * hl * s * wl * s
        n_sub, n_fold = _launches(shapes, part, m_lo, c, 4 * c), _launches(shapes, part, 4 * m_lo, c, 9 * c)
        if l in subpixel:
            assert (n_sub, n_fold) == (4, 0), (l, n_sub, n_fold, shapes)
        if l in folded:
            assert (n_sub, n_fold) == (0, 1), (l, n_sub, n_fold, shapes)


def check_blocks(plan, host, trace, out, idx, asd, sd64, pick, prec, tol, worst, plan32=None, k32=None, margin=None):
    """every block of the plan, teacher-forced, in float64, per image.  `host`: the plan's host inputs (fp32, the picked images),
    `trace`: name -> fp32 [picked, C, H, W] of the engine's records, `out`: the call's output, `idx`: the engine's VQ indices [picked, h*w]
    (or None), `asd` / `sd64`: the fp32 / float64 weights; returns (failures, missing).  With `plan32` (name -> step of the plan on the fp32
    weights) and `k32` the tolerance of a block and image is max(tol, k32 * err32), err32 the float32 oracle's own error there; `margin`
    (a one-element list) then receives (error, block, err32, tolerance) of the block nearest its tolerance."""
    last = plan[-1].name
    failures, missing = [], []
    if margin is not None:
        margin[:] = [(0.0, "-", float("nan"), tol), float("nan")]   # (.. , the worst err32 of any block)

    def engine(name):
        if name in host:
            return host[name]
        return out if name == last else trace.get(name)

    for s in plan:
        if s.name == "dec.idx":
            if "dec.zq.z" not in trace:
                missing.append("dec.zq.z")
                continue
            if not torch.equal(trace["dec.zq.z"], host["z"]):
                failures.append("dec.zq.z: the latents the VQ kernel saw are not the call's input")
            e64 = sd64["quantize.embedding.weight"]
            for k, b in enumerate(pick):
                differ, bad, _ = H.vq_check(trace["dec.zq.z"][k:k + 1].double(), e64, idx[k])
                worst[("dec.idx (differ)", prec)] = max(worst.get(("dec.idx (differ)", prec), 0.0), differ)
                if bad or differ > H.VQ_CAP:
                    failures.append(f"dec.idx: image {b}: {bad} wrong indices, {differ:.2e} of the positions differ from the float64 argmin (cap {H.VQ_CAP:.0e})")
            continue
        got = engine(s.name)
        if got is None:
            missing.append(s.name)
            continue
        if s.name == "dec.zq":
            # the codebook row of the ENGINE's index through the reference's fp32 expression: bit for bit
            ref = oc.vq_lookup(asd, host["z"], idx.reshape(-1).long())
            row = asd["quantize.embedding.weight"][idx.reshape(-1).long()].view(len(pick), host["z"].shape[2], host["z"].shape[3], -1).permute(0, 3, 1, 2)
            if not torch.equal(got, ref):
                failures.append(f"dec.zq: not the codebook row of the engine's index ({(got != ref).sum().item()} elements differ)")
            if not bool(((got - row).abs() <= 2.0 ** -23 * (host["z"].abs() + row.abs())).all()):
                failures.append("dec.zq: further from the codebook row than the roundings of z + (e - z)")
            continue
        ins = [engine(i) for i in s.inputs]
        if any(v is None for v in ins):
            continue   # (an input block is missing: reported above)
        ref = s.fn(*[v.double() for v in ins])
        assert ref.dtype == torch.float64 and got.shape == ref.shape, (s.name, ref.dtype, got.shape, ref.shape)
        got = got.double()
        e32 = R.err32(plan32[s.name], ins, ref) if k32 else None
        if k32 and margin is not None:
            margin[1] = max(v for v in [margin[1]] + e32 if not np.isnan(v))
        for k, b in enumerate(pick):
            e = ((got[k] - ref[k]).abs().max() / ref[k].abs().max().clamp_min(1e-30)).item()
            worst[(s.name, prec)] = max(worst.get((s.name, prec), 0.0), e)
            tol_b = max(tol, k32 * e32[k]) if k32 else tol
            if margin is not None and (not np.isfinite(e) or e / tol_b > margin[0][0] / margin[0][3]):
                margin[0] = (e, s.name, e32[k] if k32 else float("nan"), tol_b)
            if not np.isfinite(e) or e > tol_b:
                failures.append(f"{s.name}: image {b} error {e:.3e} > {tol_b:.1e}" + (f" (err32 {e32[k]:.3e})" if k32 else ""))
        del ref, got, ins
    return failures, missing


@pytest.mark.parametrize("key,call,B,h,w,prec,attn,subpixel,folded,regime", ALL_CASES,
                         ids=[f"{c[0]}-{c[1]}-B{c[2]}-{c[3]}x{c[4]}-{c[5]}" + ("" if c[9] == "base" else f"-{c[9]}") for c in ALL_CASES])
def test_every_autoencoder_block_against_float64(gpu, key, call, B, h, w, prec, attn, subpixel, folded, regime):
    ap, asd, sd64, eng = _model(key, gpu, regime)
    p = parse_precision(prec)
    if call == "encode":
        x = torch.rand(B, 3, h, w, generator=torch.Generator().manual_seed(1000 + B)) * 2 - 1
        plan, hname = oc.ae_encode_plan(sd64, ap), "x"
        run = lambda: (eng.vq_encode(x.to(gpu), prec=p), None)
    else:
        x = H.vq_latents(B, int(ap["embed_dim"]), h, w, 2000 + B)
        plan, hname = oc.ae_decode_plan(sd64, ap, force_not_quantize=call == "decode_nq"), "z"
        if call == "decode":
            run = lambda: eng.vq_decode(x.to(gpu), prec=p, return_indices=True)
        else:
            run = lambda: (eng.vq_decode(x.to(gpu), force_not_quantize=True, prec=p), None)
    f = 2 ** (len(ap["ddconfig"]["ch_mult"]) - 1)
    pick = _pick(B, *((h // f, w // f) if call == "encode" else (h, w)))
    want = [s.name for s in plan] + ["dec.zq.z"]

    # the same pass untraced and traced: same bits, same network launches
    eng.debug_enable(False)
    out, idx = run()
    torch.cuda.synchronize()
    n_plain = eng.last_launch_count()
    eng.debug_enable(True)
    try:
        out_tr, idx_tr = run()
        n_traced = eng.last_launch_count()
        fam = [n for name, fl, ms, n in eng.profile_families()]
        recs = eng.debug_records()
        trace = {k: v.cpu() for k, v in eng.debug_trace(names=want, images=pick).items()}
    finally:
        eng.debug_enable(False)
    assert torch.equal(out, out_tr) and (idx is None or torch.equal(idx, idx_tr)), "a traced pass computes something else than an untraced one"
    assert n_plain == n_traced, (n_plain, n_traced)
    names = [n for n, _ in recs]
    assert len(set(names)) == len(names), names
    if call == "decode_nq":
        assert not any(n.startswith("dec.zq") for n in names), names
    cap = sum(-(-int(np.prod(d)) * 4 // 256) * 256 for _, d in recs)
    # ... and once more with the profiler's brackets, for the launch shapes: still the same bits
    eng.profile_enable(True)
    try:
        out_pr, _ = run()
        torch.cuda.synchronize()
        shapes, _ = eng.profile_shapes()
    finally:
        eng.profile_enable(False)
    assert torch.equal(out, out_pr)
    kernels = None
    try:
        check_kernels(ap, call, B, h, w, attn, subpixel, folded, fam, shapes)
    except AssertionError as err:   # (reported after the blocks, so that one run shows both)
        kernels = err

    host = {hname: x[pick]}
    idx_p = idx.view(B, -1)[pick].cpu() if call == "decode" else None
    own = {}
    if regime == "base":
        failures, missing = check_blocks(plan, host, trace, out[pick].cpu(), idx_p, asd, sd64, pick, prec, TOL[prec], own)
    else:   # a regime case: in fp32 and split storage the tolerance follows the float32 oracle's own error on the block
        k32, margin = R.K32.get(prec), []
        plan32 = {s.name: s for s in (oc.ae_encode_plan(asd, ap) if call == "encode" else oc.ae_decode_plan(asd, ap))} if k32 else None
        failures, missing = check_blocks(plan, host, trace, out[pick].cpu(), idx_p, asd, sd64, pick, prec, TOL[prec], own, plan32, k32, margin)
        _worst_regime[(regime, call, prec)] = margin[0] + (margin[1],)
        print(f"\n{regime} {call} {prec}: block nearest its tolerance {margin[0][1]}: error {margin[0][0]:.3e}, err32 {margin[0][2]:.3e}, "
              f"tolerance {margin[0][3]:.3e}; worst err32 of any block {margin[1]:.3e}")
    for k, v in (own.items() if regime == "base" else ()):
        _worst[k] = max(_worst.get(k, 0.0), v) if np.isfinite(v) else v
    own_e, own_n = max(((v, n) for (n, _), v in own.items() if not n.startswith("dec.idx")), default=(0.0, "-"))
    worst = max((v for (n, pp), v in _worst.items() if pp == prec and not n.startswith("dec.idx")), default=0.0)
    print(f"\n{key} {call} B={B} {h}x{w} {prec}: {len(plan)} blocks x {len(pick)} images, {n_traced} launches, {len(recs)} records, capture region "
          f"{cap / 2 ** 30:.2f} GiB, worst error of this case {own_e:.3e} ({own_n}), VQ positions differing {own.get(('dec.idx (differ)', prec), 0.0):.2e}, "
          f"worst {prec} error so far {worst:.3e}")
    assert not missing, f"blocks of the plan missing from the trace: {missing}"
    assert not failures, "\n".join(failures[:40])
    if kernels is not None:
        raise kernels

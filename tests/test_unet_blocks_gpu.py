"""Every UNet block of the production kernel graph against float64, teacher-forced, per image.

The engine runs its own kernel choice at each batch (Winograd on the 64 x 64 / 32 x 32 levels at the bench batch, split-K small-plane
halo kernels, GroupNorm tails and folds, fused qkv attention, the fused Swin MLP with the patch-unembed fold, the shortcut fold, the
sub-pixel upsampling conv, the fused head, a per-image FiLM table at mixed timesteps).  A traced call (Engine.debug_enable) runs that same
graph - the test asserts it: same output bits, same launch count - and records every block boundary.  Each block of the plan
(oracle/resshift_oracle.py: unet_plan) is then fed the engine's own recorded inputs in float64 and compared with the engine's output of
that block, per image: max |engine - ref| / max |ref| over the image's block output, so that one image reading another image's FiLM row
cannot hide behind another image's scale, and errors do not build up along the chain.  Run with -s for the table of the worst error per
block and precision (the margin later kernel changes have left) and the case each is from.

The kernel choice follows the shape as well as the batch, so the cases are the bench's square shapes and what the tile pool and the default
tiled path hand the UNet: non-square size classes (a transposed H / W in slab counts, arrival counts of GroupNorm tails, the row-band shift
mask, the sub-pixel row scatter, window counts or the feature extractor's dims cannot pass there), a plane larger than the constructed one,
batch 1, and the batch at which the small-plane halo kernel splits K deepest.  Each of those asserts that it ran the kernels it is there for."""
import numpy as np
import pytest
import torch

import _regimes as R
import helpers as H
from oracle import resshift_oracle as oc
from resshift_amd.config import load_config, to_plain
from resshift_amd.engine import Engine, parse_precision
from resshift_amd.spec import unet_param_spec

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

CONFIGS = {"realsr": "realsr_swinunet_realesrgan256", "faceir": "faceir_gfpgan512_lpips", "inpaint": "inpaint_lama256_imagenet"}
# (net, batch, latent h, w - None: the config's image_size, the bench shape -, storage, timesteps, what the case must have run).  The lq and mask
# size follows from the latent size by the config's lq_size / image_size ratio.  The first eleven are the bench shapes; the rest are what the
# tile pool and the default tiled path (chop_size 128, chop_bs 1) hand the UNet: the padded size classes at whatever batch the pool has, the
# smallest shapes that reach each kernel path (four levels and 8-pixel windows want multiples of 64: 64 x 128 is the smallest non-square plane).
# "what it must have run": kernel families with at least one launch in the traced pass ("wino", "halo_split", "halo16"), and "subpixel" /
# "folded": the 32 x 64 -> 64 x 128 upsampling conv as four sub-pixel launches (8 * 32 * 64 = 16384 low-resolution pixels: exactly the
# threshold) / not as those (6 * 64 * 32 = 12288).
CASES = [("realsr", 32, None, None, "split", "mixed", ("wino10",)), ("realsr", 32, None, None, "fp16", "mixed", ()),
         ("realsr", 32, None, None, "fp32", "mixed", ()), ("realsr", 32, None, None, "split", "shared", ("wino10",)),
         ("realsr", 3, None, None, "split", "mixed", ()), ("realsr", 3, None, None, "fp16", "mixed", ()), ("realsr", 3, None, None, "fp32", "mixed", ()),
         ("faceir", 16, None, None, "split", "mixed", ()), ("faceir", 16, None, None, "fp16", "mixed", ()),
         ("inpaint", 16, None, None, "split", "mixed", ()), ("inpaint", 16, None, None, "fp16", "mixed", ()),
         ("realsr", 8, 64, 128, "split", "mixed", ("wino", "halo_split", "subpixel")),   # wide planes; fused MLP x 8
         ("realsr", 6, 128, 64, "split", "mixed", ("wino", "halo_split", "folded")),     # the tall counterpart
         ("realsr", 6, 64, 128, "fp16", "mixed", ("halo16",)),                           # halo fp16 and the fp16 fused kernels on wide planes
         ("realsr", 2, 64, 128, "fp32", "mixed", ()),                                    # exact path, non-square
         ("realsr", 1, 128, 128, "split", "shared", ()),                                 # the default tile of the default tiled path
         ("realsr", 1, 64, 64, "split", "shared", ()), ("realsr", 1, 64, 64, "fp16", "shared", ()),   # batch 1
         ("realsr", 4, 64, 64, "split", "mixed", ("halo_split",)),                       # small-plane halo kernel, few tiles, deepest split-K
         ("inpaint", 2, 64, 128, "split", "mixed", ()),                                  # mask concat on a non-square plane
         ("faceir", 1, 64, 128, "split", "shared", ())]                                  # feature extractor on 512 x 1024
FAMILY = {"wino": "wino_kernel", "wino10": "wino_kernel", "halo_split": "igemm4_kernel<*, true>", "halo16": "igemm4_kernel<*, false>"}   # Engine.FAMILIES
# Per-image tolerance of every block, per precision: under 3x the worst error measured over the bench shapes (the first eleven CASES) on the
# MI355X.  Measured there (worst block): split 1.79e-6 (head; the upsampling convs out.2 / out.5 1.4e-6 / 1.0e-6, every other block
# <= 1.2e-6), fp16 8.8e-4 (in.1, fp16 storage of the block output), fp32 3.6e-6 (the upsampling convs out.2 / out.5 / out.8: 3.6e-6 /
# 2.7e-6 / 3.2e-6 - K = 9 x 640 products in one fp32 sum -, every other block <= 1.9e-6).
# The tile pool's shapes (the last ten CASES) run the same kernel families and reduction lengths and keep these bounds; no block needed one
# of its own.  Measured over them (worst block of the worst case): split 1.73e-6 (head, B = 8 at 64 x 128; the head is the worst block of
# every split case but faceir's, 1.15e-6 .. 1.73e-6), fp16 9.07e-4 (in.1, B = 6 at 64 x 128: the fp16 rounding of the block output again,
# 2.8x under the bound; batch 1: 7.6e-4, mid.swin), fp32 3.11e-6 (out.8, B = 2 at 64 x 128).
TOL = {"split": 5e-6, "fp16": 2.5e-3, "fp32": 1e-5}
# The weight regimes (oracle/synth.py: regime_state_dict; what each exercises is pinned on the CPU, tests/test_unet_blocks_cpu.py): the cases
# above all load one draw, in which no GroupNorm variance comes within 1e4 of eps, no softmax is peaked and no GELU argument leaves |x| < 7.
# "quiet" (variances around and far below eps), "loud" (peaked softmaxes, logits to 200, GELU arguments to 30, SiLU far out on both sides) and
# "zero_init" (the reference's initial state: every ResBlock's second conv and the head conv exactly zero) run the smallest shape the net
# accepts: realsr, B = 3, 64 x 64, mixed timesteps.  The tolerance of a block there is max(TOL[prec], k * err32): err32 is the same plan step
# evaluated by the oracle in float32 on the same teacher-forced inputs against its float64 value, per image, the same max-norm - the
# reference's own arithmetic, never the engine's (it stays <= 1e-4 on every block: asserted on the CPU) - with k = 4 for fp32 storage
# (another summation order, x 2 margin) and k = 8 for split (the pair keeps 2^-22 of an operand, 4 x fp32's unit, x 2 margin).  fp16 storage
# keeps TOL["fp16"], and is left out of loud: with logits of 50 .. 200 the fp16 rounding of q and k inside a block moves probabilities by
# percents - conditioning, not a kernel property (tests/test_engine_gpu.py: test_fp16_error_on_natural_images_is_conditioning_not_a_kernel
# makes the same point).  zero_init also asserts, in all three storages, that every ResBlock without a skip conv hands back its input bit
# for bit and that the UNet's output is exactly zero.
# Measured on the MI355X (the block nearest its tolerance: error / err32; k * err32 stayed under TOL[prec] everywhere, so TOL[prec] applied):
# quiet split 1.67e-6 / 2.8e-7 (head), fp16 8.05e-4 (in.2), fp32 1.44e-6 / 3.4e-7 (head); loud split 2.20e-6 / 3.6e-7 (head), fp32 2.27e-6 /
# 1.87e-6 (in.1: the float32 oracle is no better there); zero_init split 5.3e-7 / 2.6e-7 (out.7), fp16 9.54e-4 (in.1), fp32 1.14e-6 / 2.6e-7
# (out.9.res).  The identity blocks and the zero output held bit for bit in all three storages.
REGIME_CASES = [("realsr", 3, 64, 64, prec, "mixed", ("families",) if prec == "split" and regime != "zero_init" else (), regime)
                for regime, precs in (("quiet", ("split", "fp16", "fp32")), ("loud", ("split", "fp32")), ("zero_init", ("split", "fp16", "fp32")))
                for prec in precs]
ALL_CASES = [c + ("base",) for c in CASES] + REGIME_CASES
# the kernel families with at least one launch in the traced realsr split pass at B = 3, 64 x 64 (from a traced run of the build these
# cases were added to): a quiet or loud split case must have run each of them
FAMILIES_B3 = ("igemm_split_kernel (implicit GEMM, split storage)",                                        # 119 launches there
               "win_attn_qkv_split_kernel (fused qkv + window attention + proj, split storage)")          # 18
# (at this batch the Swin MLPs run as two implicit GEMMs with the GELU in fc1's epilogue, and no conv takes the halo or Winograd kernels:
# the fused MLP's GELU and the attention, GroupNorm and softmax kernels meet the same operand ranges in tests/test_ops_regimes_gpu.py)

_models = {}
_worst = {}   # (block, prec) -> (worst per-image error over the base cases run so far, the case it is from)
_worst_regime = {}   # (regime, prec) -> (error of the block and image nearest its tolerance, block, its err32 or NaN, tolerance applied, worst err32)
_PIXELS = 8 * 64 * 64   # latent pixels of the images compared per case: what the float64 side of the batch-32 bench case costs


@pytest.fixture(scope="module", autouse=True)
def _table():
    """after the module: the table of the worst per-image error per block and precision over every case that ran (-s)"""
    yield
    if not _worst:
        return
    precs = [p for p in TOL if any(pp == p for _, pp in _worst)]
    names = list(dict.fromkeys(n for n, _ in _worst))
    nan = (float("nan"), "-")
    print("\nworst per-image error per block (max |engine - float64| / max |float64|, teacher-forced), and the case it is from:")
    print(f"{'block':<12}" + "".join(f"{p:>12}" for p in precs) + "   " + " | ".join(precs))
    for n in names:
        print(f"{n:<12}" + "".join(f"{_worst.get((n, p), nan)[0]:>12.3e}" for p in precs) + "   " + " | ".join(_worst.get((n, p), nan)[1] for p in precs))
    print(f"{'worst':<12}" + "".join(f"{max(v for (n, pp), (v, _) in _worst.items() if pp == p):>12.3e}" for p in precs))
    print(f"{'tolerance':<12}" + "".join(f"{TOL[p]:>12.1e}" for p in precs))
    if _worst_regime:
        print("\nweight regimes (realsr, B = 3, 64 x 64): the block and image nearest its tolerance - error, the float32 oracle's error there (err32), "
              "tolerance applied - and the worst err32 of any block:")
        for (regime, prec), (e, name, e32, tol, w32) in _worst_regime.items():
            print(f"{regime:<10}{prec:<6}{e:>12.3e} ({name}){e32:>12.3e}{tol:>12.3e}{w32:>12.3e}")
    _models.clear()


def _model(key, gpu, regime="base"):
    """one Engine per (config, regime)"""
    key, cname = (key, regime), key
    if key not in _models:
        cfg = to_plain(load_config(CONFIGS[cname]))
        up, dp = cfg["model"]["params"], cfg["diffusion"]["params"]
        uspec, _ = unet_param_spec(up)
        usd = R.regime_sd(H.synth.synthetic_state_dict(uspec, H.SEED_W, image_size=up["image_size"]), regime)
        sd64 = {k: (v.double() if torch.is_floating_point(v) else v) for k, v in usd.items()}
        eng = Engine(unet_params=up, ae_params=None, device=gpu)
        eng.load_state_dicts(unet_sd=usd)
        eng.mark_weights_ready()
        _models[key] = (up, int(dp["steps"]), sd64, eng, usd)
    return _models[key]


def _pick(B, h=64, w=64):
    """images spread over the batch, the first and the last included, as many as the pixel budget allows: 8 at 64 x 64, 4 at 64 x 128, 2 at
    128 x 128 (all of a smaller batch)"""
    return sorted(set(int(v) for v in np.linspace(0, B - 1, min(B, max(2, _PIXELS // (h * w)))).round()))


def _worse(e, cur):
    """e is a worse error than cur (a NaN is the worst there is, and stays)"""
    return not np.isnan(cur) and (np.isnan(e) or e > cur)


def _id(key, B, h, w, prec, ts, need=(), regime="base"):
    return f"{key}-B{B}-" + (f"{h}x{w}-" if h else "") + f"{prec}-{ts}" + ("" if regime == "base" else f"-{regime}")


@pytest.mark.parametrize("key,B,h,w,prec,ts,need,regime", ALL_CASES, ids=[_id(*c) for c in ALL_CASES])
def test_every_unet_block_against_float64(gpu, key, B, h, w, prec, ts, need, regime):
    up, T, sd64, eng, usd = _model(key, gpu, regime)
    case = _id(key, B, h, w, prec, ts, (), regime)
    hz, hl = int(up["image_size"]), int(up["lq_size"])
    h, w = (hz, hz) if h is None else (h, w)
    lh, lw = h * hl // hz, w * hl // hz
    g = torch.Generator().manual_seed(1000 + B)
    x = torch.randn(B, int(up["in_channels"]), h, w, generator=g)
    lq = torch.rand(B, 3, lh, lw, generator=g) * 2 - 1
    mask = ((torch.rand(B, 1, lh, lw, generator=g) > 0.6).float() * 2 - 1) if up.get("cond_mask") else None
    t = [(7 * b) % T for b in range(B)] if ts == "mixed" else [7 % T] * B
    args = dict(lq=lq.to(gpu), mask=mask.to(gpu) if mask is not None else None, prec=parse_precision(prec))

    # the same pass untraced and traced: same bits, same network launches
    eng.debug_enable(False)
    out = eng.unet_forward(x.to(gpu), t, **args)
    torch.cuda.synchronize()
    n_plain = eng.last_launch_count()
    eng.debug_enable(True)
    try:
        out_tr = eng.unet_forward(x.to(gpu), t, **args)
        n_traced = eng.last_launch_count()
        fam = {name: n for name, fl, ms, n in eng.profile_families()}
        pick = _pick(B, h, w)
        trace = {k: v[pick].double().cpu() for k, v in eng.debug_trace().items()}
    finally:
        eng.debug_enable(False)
    assert torch.equal(out, out_tr), "a traced pass computes something else than an untraced one"
    assert n_plain == n_traced, (n_plain, n_traced)
    # the traced pass ran the kernels the case is there for (the exact mix is pinned on the CPU: tests/test_host_cpu.py)
    if "families" in need:
        assert FAMILIES_B3 and not [f for f in FAMILIES_B3 if not fam.get(f)], ([f for f in FAMILIES_B3 if not fam.get(f)], fam)
    for what in need:
        if what in FAMILY:
            nl = [n for name, n in fam.items() if name.startswith(FAMILY[what])]
            assert nl and nl[0] >= (10 if what == "wino10" else 1), (what, fam)   # (wino10: the bench batch's Winograd levels)
    if "subpixel" in need or "folded" in need:
        # ... and once more with the profiler's brackets, for the launch shapes: still the same bits.  The last upsampling step, h/2 x w/2 ->
        # h x w at C = model_channels * channel_mult[1]: four launches over the low-resolution grid with K = 2 * 2 * C, or none of them
        eng.profile_enable(True)
        try:
            out_pr = eng.unet_forward(x.to(gpu), t, **args)
            torch.cuda.synchronize()
            shapes, _ = eng.profile_shapes()
        finally:
            eng.profile_enable(False)
        assert torch.equal(out, out_pr)
        c, m_lo = int(up["model_channels"]) * int(up["channel_mult"][1]), B * (h // 2) * (w // 2)
        n_sub = sum(s["launches"] for s in shapes if s["part"] == "unet" and (s["M"], s["N"], s["K"]) == (m_lo, c, 4 * c))
        assert n_sub == (4 if "subpixel" in need else 0), (n_sub, shapes)

    # every block of the plan, teacher-forced, in float64, per image
    host = {"x": x[pick].double(), "t": torch.tensor([t[b] for b in pick]), "lq": lq[pick].double()}
    if mask is not None:
        host["mask"] = mask[pick].double()
    plan = oc.unet_plan(sd64, up, with_lq=True, with_mask=mask is not None)
    k32 = R.K32.get(prec) if regime != "base" else None   # (a regime case in fp32 or split storage: the tolerance follows the float32 oracle's own error)
    plan32 = {s.name: s for s in oc.unet_plan(usd, up, with_lq=True, with_mask=mask is not None)} if k32 else None
    own_regime, w32 = (0.0, "-", float("nan"), TOL[prec]), float("nan")
    got_head = out[pick].double().cpu()
    env = dict(host)
    failures, missing, own = [], [], (0.0, "-")
    for s in plan:
        if s.name != "emb" and s.name != "head" and s.name not in trace:
            missing.append(s.name)
            continue
        ins = [env[i] if i in env else trace.get(i) for i in s.inputs]
        if any(v is None for v in ins):
            continue   # (an input block is missing: reported above)
        ref = s.fn(*ins)
        if s.name == "emb":
            env["emb"] = ref
            continue
        got = got_head if s.name == "head" else trace[s.name]
        assert got.shape == ref.shape, (s.name, got.shape, ref.shape)
        e32 = R.err32(plan32[s.name], ins, ref) if k32 else None
        w32 = max([v for v in [w32] + (e32 or []) if not np.isnan(v)], default=float("nan"))
        if regime == "zero_init" and (s.name == "head" or R.unet_identity_step(s, sd64)):
            # the reference's initial state: the zeroed second conv leaves the shortcut alone, the zeroed head conv gives zero - exactly
            want = torch.zeros_like(got) if s.name == "head" else ins[0]
            if not torch.equal(got, want):
                failures.append(f"{s.name}: not bit for bit " + ("zero" if s.name == "head" else f"its input {s.inputs[0]}") +
                                f" ({(got != want).sum().item()} elements differ, by up to {(got - want).abs().max().item():.3e})")
        for k, b in enumerate(pick):
            e = ((got[k] - ref[k]).abs().max() / ref[k].abs().max().clamp_min(1e-30)).item()
            tol = max(TOL[prec], k32 * e32[k]) if k32 else TOL[prec]
            if _worse(e, own[0]):
                own = (e, s.name)
            if regime == "base" and _worse(e, _worst.get((s.name, prec), (0.0, ""))[0]):
                _worst[(s.name, prec)] = (e, case)
            if regime != "base" and _worse(e / tol, own_regime[0] / own_regime[3]):
                own_regime = (e, s.name, e32[k] if k32 else float("nan"), tol)
            if not np.isfinite(e) or e > tol:
                failures.append(f"{s.name}: image {b} (t={t[b]}) error {e:.3e} > {tol:.1e}" + (f" (err32 {e32[k]:.3e})" if k32 else ""))
    if regime != "base":
        _worst_regime[(regime, prec)] = own_regime + (w32,)
        print(f"\n{case}: block nearest its tolerance {own_regime[1]}: error {own_regime[0]:.3e}, err32 {own_regime[2]:.3e}, tolerance {own_regime[3]:.3e}; "
              f"worst err32 of any block {w32:.3e}")
    worst = max((v for (n, p), (v, _) in _worst.items() if p == prec), default=0.0)
    print(f"\n{key} B={B} {h}x{w} {prec} {ts}: {len(plan) - 1} blocks x {len(pick)} images, {n_traced} launches, worst error of this case "
          f"{own[0]:.3e} ({own[1]}), worst {prec} error so far {worst:.3e}")
    assert not missing, f"blocks of the plan missing from the trace: {missing}"
    assert not failures, "\n".join(failures[:40])

"""The UNet's block plan (oracle/resshift_oracle.py: unet_plan) and the engine's debug trace, without a GPU.

tests/test_unet_blocks_gpu.py checks every block of the production kernel graph against a float64 reference, teacher-forced: each block of
the plan is fed the engine's own recorded inputs.  That rests on three things checked here: the plan chained is the oracle's forward, the
plan runs in float64 when given float64 weights and inputs, and the engine records exactly the plan's block names, once each, with the
plan's dims - without changing the launches of the pass it observes."""
import os
import re
import subprocess
import sys

import pytest
import torch

import _regimes as R
import helpers as H
from oracle import resshift_oracle as oc
from resshift_amd.config import load_config, to_plain
from resshift_amd.spec import unet_param_spec

torch.set_grad_enabled(False)

NO_GPU = {"HIP_VISIBLE_DEVICES": "-1"}


def _inputs(tag):
    """(params, fp32 state_dict, host inputs) of a tiny case or of the realsr config at B=1 ("realsr": its own 64 x 64 latent,
    "realsr@64x128": a non-square one)"""
    if tag.startswith("realsr"):
        up, ap, dp = H.realsr_params()
        usd, _ = H.weights(up, ap)
        h, w = (int(v) for v in tag.split("@")[1].split("x")) if "@" in tag else (64, 64)
        y, noises, _ = H.synth.synthetic_inputs(H.SEED_X, 1, h, w, 3, h, w, dp["steps"])
        return up, usd, {"x": noises[1] * 1.3, "t": torch.tensor([7]), "lq": y, "mask": None}, "realsr/unet"
    up, ap, dp, with_mask = H.CASES[tag]
    usd, _ = H.weights(up, ap)
    y, noises, mask = H.case_inputs(up, ap, dp, with_mask)
    return up, usd, {"x": noises[1] * 1.3, "t": torch.tensor([2, 2]), "lq": y, "mask": mask if with_mask else None}, f"{tag}/unet"


def _teacher_forced(plan, env):
    """every step of the plan on its own, fed clones of the stored outputs of the steps it reads (the GPU test's pattern)"""
    out = {}
    for s in plan:
        out[s.name] = s.fn(*[env[i].clone() for i in s.inputs])
    return out


@pytest.mark.parametrize("tag", ["tiny", "tiny_fe", "tiny_fe8", "realsr"])
def test_plan_reproduces_unet_forward_bit_for_bit(tag):
    up, usd, inp, golden = _inputs(tag)
    ref = oc.unet_forward(usd, up, **inp)
    plan = oc.unet_plan(usd, up, with_lq=True, with_mask=inp["mask"] is not None)
    names = [s.name for s in plan]
    assert len(set(names)) == len(names) and names[0] == "emb" and names[-1] == "head", names
    env = oc.run_plan(plan, {k: v for k, v in inp.items() if v is not None})
    assert torch.equal(env["head"], ref)
    # each block alone, from the stored outputs of its inputs: the same bits (a step reads nothing but its declared inputs)
    tf = _teacher_forced(plan, env)
    for n in names:
        assert torch.equal(tf[n], env[n]), n
    # and the chain is still the reference's forward (the fixture of test_oracle.py)
    assert H.rel_err(ref, torch.from_numpy(H.golden()[golden])) < 2e-5


@pytest.mark.parametrize("tag", ["tiny_fe", "realsr", "realsr@64x128"])
def test_plan_in_float64(tag):
    """float64 weights and inputs keep every step in float64 (GroupNorm and the timestep embedding included), and the result agrees
    with the fp32 oracle to fp32 round-off"""
    up, usd, inp, _ = _inputs(tag)
    sd64 = {k: (v.double() if torch.is_floating_point(v) else v) for k, v in usd.items()}
    in64 = {k: (v.double() if v is not None and torch.is_floating_point(v) else v) for k, v in inp.items()}
    plan64 = oc.unet_plan(sd64, up, with_lq=True, with_mask=inp["mask"] is not None)
    env64 = oc.run_plan(plan64, {k: v for k, v in in64.items() if v is not None})
    env32 = oc.run_plan(oc.unet_plan(usd, up, with_lq=True, with_mask=inp["mask"] is not None), {k: v for k, v in inp.items() if v is not None})
    worst = 0.0
    for s in plan64:
        a, b = env64[s.name], env32[s.name]
        assert a.dtype == torch.float64, (s.name, a.dtype)
        e = ((a - b.double()).abs().max() / a.abs().max()).item()
        worst = max(worst, e)
        assert e < 2e-5, (s.name, e)
    # really float64 arithmetic, not float32 values in a float64 container: the result does not round-trip through float32
    out = env64["head"]
    assert (out.float().double() != out).float().mean().item() > 0.9
    assert worst > 0.0
    print(f"{tag}: float64 plan vs fp32 oracle, worst step {worst:.2e}")


def _plan_dims(cname, B, h=None, w=None):
    """name -> (B, C, H, W) of every traced step of the plan (fp32 oracle at batch 1, synthetic weights) at the latent size h x w (the
    config's image_size by default; the lq / mask size follows by the config's lq_size / image_size ratio)"""
    up = to_plain(load_config(cname))["model"]["params"]
    uspec, _ = unet_param_spec(up)
    usd = H.synth.synthetic_state_dict(uspec, H.SEED_W, image_size=up["image_size"])
    hz, hl = int(up["image_size"]), int(up["lq_size"])
    h, w = (hz, hz) if h is None else (h, w)
    lh, lw = h * hl // hz, w * hl // hz
    g = torch.Generator().manual_seed(5)
    env = {"x": torch.randn(1, int(up["in_channels"]), h, w, generator=g), "t": torch.tensor([3]),
           "lq": torch.rand(1, 3, lh, lw, generator=g) * 2 - 1}
    if up.get("cond_mask"):
        env["mask"] = (torch.rand(1, 1, lh, lw, generator=g) > 0.5).float() * 2 - 1
    plan = oc.unet_plan(usd, up, with_lq=True, with_mask="mask" in env)
    env = oc.run_plan(plan, env)
    return {s.name: (B,) + tuple(env[s.name].shape[1:]) for s in plan if s.name not in ("emb", "head")}


_R, _F, _I = "realsr_swinunet_realesrgan256", "faceir_gfpgan512_lpips", "inpaint_lama256_imagenet"
# (config, batch, precision 0 fp16 | 1 fp32 | 2 split, latent h, w - None: image_size); from the fifth row on: the tile pool's size classes and
# batch 1, the cases tests/test_unet_blocks_gpu.py adds to the square bench shapes
FAKE = [(_R, 32, 2, None, None), (_R, 3, 0, None, None), (_F, 2, 2, None, None), (_I, 4, 1, None, None),
        (_R, 8, 2, 64, 128), (_R, 6, 2, 128, 64), (_R, 6, 0, 64, 128), (_R, 2, 1, 64, 128), (_R, 1, 2, 128, 128), (_R, 1, 2, 64, 64),
        (_R, 1, 0, 64, 64), (_R, 4, 2, 64, 64), (_I, 2, 2, 64, 128), (_F, 1, 2, 64, 128)]


@pytest.mark.parametrize("cname,B,prec,h,w", FAKE, ids=[f"{c}-{b}-{p}" + (f"-{h}x{w}" if h else "") for c, b, p, h, w in FAKE])
def test_trace_names_are_the_plan_blocks_without_a_gpu(cname, B, prec, h, w):
    """RS_FAKE_DEVICE=1 (test-hooks library, see _fake_device_plumbing.py): a traced rs_unet_forward at mixed timesteps records every
    block of the plan exactly once, with the plan's dims, plus inner records under a block's prefix; and tracing leaves the pass alone -
    the same launch count, pool, tickets and sequence numbers as the untraced call."""
    from resshift_amd import build as _b

    env = dict(os.environ, RS_FAKE_DEVICE="1", RESSHIFT_HIP_LIB=_b.build_testhooks(), **NO_GPU)
    r = subprocess.run([sys.executable, os.path.join(H.ROOT, "tests", "_fake_device_trace.py"), cname, str(B), str(prec)] +
                       ([str(h), str(w)] if h else []), env=env,
                       capture_output=True, text=True, timeout=600)
    fake = re.findall(r"\[fake device\] (dry: .*)", r.stderr)
    calls = re.findall(r"CALL (\w+) rc -?\d+ launches (\d+) records (\d+)", r.stdout)
    assert len(fake) == 2 and len(calls) == 2, (r.stdout[-800:], r.stderr[-1500:])
    assert fake[0] == fake[1], fake                                  # dry / real bookkeeping of the two calls
    assert calls[0][1] == calls[1][1] and int(calls[0][2]) == 0, calls   # network launches; no records untraced
    recs = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("REC ")]
    assert len(recs) == int(calls[1][2]) and recs, calls
    names = [n for n, *_ in recs]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    dims = _plan_dims(cname, B, h, w)
    blocks = {n: tuple(int(v) for v in d) for n, *d in recs if n in dims}
    assert set(blocks) == set(dims), (sorted(set(dims) - set(blocks)), sorted(set(blocks) - set(dims)))
    for n, d in dims.items():
        assert blocks[n] == d, (n, blocks[n], d)
    # every other record is an inner one, named under the prefix of a block of the plan
    for n in names:
        if n not in dims:
            parts = n.split(".")
            assert any(".".join(parts[:k]) in dims for k in range(1, len(parts))), n


# ---------------------------------------------------------------- the weight regimes of tests/test_unet_blocks_gpu.py (oracle/synth.py: regime_state_dict)
def test_regime_state_dict_is_a_pure_function_of_the_synthetic_weights():
    up, ap, dp = H.realsr_params()
    usd, _ = H.weights(up, ap)
    before = {k: v.clone() for k, v in usd.items()}
    zero = set(H.synth.zero_module_names(usd.keys()))
    nres = sum(k.endswith(".in_layers.0.weight") for k in usd)
    assert len(zero) == 2 * nres + 2 and "out.2.weight" in zero and "middle_block.0.out_layers.3.bias" in zero
    for regime in R.REGIMES:
        sd = H.synth.regime_state_dict(usd, regime)
        assert list(sd) == list(usd) and all(torch.equal(usd[k], before[k]) for k in usd)
        again = H.synth.regime_state_dict(usd, regime)
        for k, v in sd.items():
            assert v.shape == usd[k].shape and v.dtype == usd[k].dtype and torch.equal(v, again[k]), k
            if not torch.is_floating_point(v) or k.endswith("attn_mask"):
                assert torch.equal(v, usd[k]), k    # index and mask buffers
            elif regime == "zero_init":
                assert torch.equal(v, torch.zeros_like(v) if k in zero else usd[k]), k
    with pytest.raises(ValueError):
        H.synth.regime_state_dict(usd, "base")


@pytest.mark.parametrize("regime", R.REGIMES)
def test_regime_is_what_it_claims_and_its_yardstick_is_small(regime):
    """The new cases of tests/test_unet_blocks_gpu.py (realsr, B = 3, 64 x 64, mixed timesteps), oracle only.  A regime must stay what it is
    there for - quiet: GroupNorm variances of the order of eps and below; loud: peaked softmaxes, GELU arguments far past the fast form's
    clamp, conv outputs still well inside fp16 - finite, and centred enough that GroupNorm's E[x^2] - mean^2 in fp32 costs ~1e-6 at most
    (|mean| / std <= 4 over every group: (1 + R^2) 2^-24).  And the tolerance's yardstick, the float32 oracle's own error on each
    teacher-forced block, stays <= 1e-4.  zero_init: a ResBlock without a skip conv is the identity and the output is zero, bit for bit."""
    up, ap, dp = H.realsr_params()
    usd, _ = H.weights(up, ap)
    sd = R.regime_sd(usd, regime)
    sd64 = {k: (v.double() if torch.is_floating_point(v) else v) for k, v in sd.items()}
    x, lq, _, t = R.unet_case_inputs(up, 3, 64, 64, int(dp["steps"]))
    plan64, plan32 = oc.unet_plan(sd64, up), oc.unet_plan(sd, up)
    with R.probe() as p:
        env = oc.run_plan(plan64, {"x": x.double(), "t": torch.tensor(t), "lq": lq.double()})
    print(f"\n{regime}: GroupNorm var / eps median {p.median_var_eps():.3g} minimum {p.min_var_eps():.3g}, max |mean| / std {p.max_offcentre():.2f}, "
          f"median largest probability {p.median_pmax():.3f}, largest GELU argument {p.gelu:.3g}, largest |conv output| {p.conv:.3g}")
    assert p.finite and all(bool(torch.isfinite(env[s.name]).all()) for s in plan64)
    assert p.max_offcentre() <= 4.0
    if regime == "quiet":
        assert p.median_var_eps() <= 0.5
    if regime == "loud":
        assert p.median_pmax() >= 0.5 and p.gelu >= 10.0 and p.conv <= 1000.0
    worst = (0.0, "-")
    for s64, s32 in zip(plan64, plan32):
        if s64.name == "emb":
            continue
        e = max(R.err32(s32, [env[i] for i in s64.inputs], env[s64.name])) if env[s64.name].abs().max() > 0 else 0.0
        worst = max(worst, (e, s64.name))
        assert e <= R.ERR32_CAP, (s64.name, e)
    print(f"{regime}: float32 oracle against float64, teacher-forced, worst block {worst[0]:.3e} ({worst[1]})")
    if regime == "zero_init":
        assert torch.equal(env["head"], torch.zeros_like(env["head"]))
        same = [s.name for s in plan64 if R.unet_identity_step(s, sd)]
        assert len(same) >= 4, same
        for s in plan64:
            if s.name in same:
                assert torch.equal(env[s.name], env[s.inputs[0]]), s.name

"""The autoencoder's block plans (oracle/resshift_oracle.py: ae_encode_plan, ae_decode_plan) and the engine's debug trace, without a GPU.

tests/test_ae_blocks_gpu.py checks every autoencoder block of the production kernel graph against a float64 reference, teacher-forced: each
block of the plan is fed the engine's own recorded inputs.  That rests on what is checked here: the plans chained are the oracle's
vq_encode / vq_decode (bit for bit the straight-line restatement of the reference they replaced, kept below), the plans run in float64 when
given float64 weights and inputs, the fp32 oracle's VQ argmin agrees with the float64 one on latents of the kind the GPU test uses, and the
engine records exactly the plans' block names, once each, with the plans' dims - without changing the launches of the pass it observes."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _regimes as R
import helpers as H
from oracle import resshift_oracle as oc
from resshift_amd.config import load_config, to_plain
from resshift_amd.spec import ae_param_spec

torch.set_grad_enabled(False)

NO_GPU = {"HIP_VISIBLE_DEVICES": "-1"}
CONFIGS = {"realsr": "realsr_swinunet_realesrgan256", "faceir": "faceir_gfpgan512_lpips"}


def _straight_encode(sd, p, x):
    """ldm/models/autoencoder.py:28-31 + Encoder.forward model.py:522-547 in one piece (vq_encode as it was before the plan)"""
    dd = p["ddconfig"]
    mult = [int(m) for m in dd["ch_mult"]]
    nrb = oc._listify(dd["num_res_blocks"], len(mult))
    h = oc._conv(sd, "encoder.conv_in", x, padding=1)
    for l in range(len(mult)):
        for i in range(nrb[l]):
            h = oc._resnet(sd, f"encoder.down.{l}.block.{i}", h)
        if l != len(mult) - 1:
            h = oc._conv(sd, f"encoder.down.{l}.downsample.conv", F.pad(h, (0, 1, 0, 1)), stride=2)
    h = oc._resnet(sd, "encoder.mid.block_1", h)
    h = oc._attn_block(sd, "encoder.mid.attn_1", h)
    h = oc._resnet(sd, "encoder.mid.block_2", h)
    h = oc._conv(sd, "encoder.conv_out", F.silu(oc._gn(sd, "encoder.norm_out", h, 1e-6)), padding=1)
    return oc._conv(sd, "quant_conv", h)


def _straight_decode(sd, p, h, force_not_quantize=False):
    """ldm/models/autoencoder.py:33-40 + quantize.py:271-312 + Decoder.forward model.py:627-660 in one piece (vq_decode as it was before
    the plan); returns (image, indices or None)"""
    dd = p["ddconfig"]
    mult = [int(m) for m in dd["ch_mult"]]
    nrb = oc._listify(dd["num_res_blocks"], len(mult))
    idx = None
    if not force_not_quantize:
        e = sd["quantize.embedding.weight"]
        zp = h.permute(0, 2, 3, 1).contiguous()
        zf = zp.view(-1, e.shape[1])
        d = torch.sum(zf ** 2, dim=1, keepdim=True) + torch.sum(e ** 2, dim=1) - 2 * torch.einsum("bd,dn->bn", zf, e.t())
        idx = torch.argmin(d, dim=1)
        zq = e[idx].view(zp.shape)
        h = (zp + (zq - zp)).permute(0, 3, 1, 2).contiguous()
    h = oc._conv(sd, "post_quant_conv", h)
    h = oc._conv(sd, "decoder.conv_in", h, padding=1)
    h = oc._resnet(sd, "decoder.mid.block_1", h)
    h = oc._attn_block(sd, "decoder.mid.attn_1", h)
    h = oc._resnet(sd, "decoder.mid.block_2", h)
    for l in reversed(range(len(mult))):
        for i in range(nrb[l] + 1):
            h = oc._resnet(sd, f"decoder.up.{l}.block.{i}", h)
        if l != 0:
            h = oc._conv(sd, f"decoder.up.{l}.upsample.conv", F.interpolate(h, scale_factor=2.0, mode="nearest"), padding=1)
    return oc._conv(sd, "decoder.conv_out", F.silu(oc._gn(sd, "decoder.norm_out", h, 1e-6)), padding=1), idx


def _inputs(tag):
    """(ae params, fp32 state_dict, image, latent, golden tag or None): the inputs of tests/test_oracle.py for the tiny cases, a 64 x 64
    image and a 16 x 16 latent (noise of scale 0.7) for the realsr autoencoder"""
    if tag == "realsr":
        up, ap, dp = H.realsr_params()
        _, asd = H.weights(up, ap)
        g = torch.Generator().manual_seed(11)
        return ap, asd, torch.rand(1, 3, 64, 64, generator=g) * 2 - 1, torch.randn(1, int(ap["embed_dim"]), 16, 16, generator=g) * 0.7, None
    up, ap, dp, with_mask = H.CASES[tag]
    _, asd = H.weights(up, ap)
    _, noises, _ = H.case_inputs(up, ap, dp, with_mask)
    img = torch.from_numpy(np.random.Generator(np.random.PCG64(7)).random((2, 3, 64, 64), dtype=np.float32) * 2 - 1)
    return ap, asd, img, noises[2] * 0.8, tag


def _teacher_forced(plan, env):
    """every step of the plan on its own, fed clones of the stored outputs of the steps it reads (the GPU test's pattern)"""
    return {s.name: s.fn(*[env[i].clone() for i in s.inputs]) for s in plan}


@pytest.mark.parametrize("tag", ["tiny", "tiny_fe8", "realsr"])
def test_plans_reproduce_vq_encode_and_vq_decode_bit_for_bit(tag):
    ap, asd, img, z, golden = _inputs(tag)
    g = H.golden()
    # encoder
    plan = oc.ae_encode_plan(asd, ap)
    names = [s.name for s in plan]
    assert len(set(names)) == len(names) and names[0] == "enc.in" and names[-2:] == ["enc.out", "enc.z"], names
    env = oc.run_plan(plan, {"x": img})
    ref = _straight_encode(asd, ap, img)
    assert torch.equal(env["enc.z"], ref) and torch.equal(oc.vq_encode(asd, ap, img), ref)
    tf = _teacher_forced(plan, env)
    for n in names:
        assert torch.equal(tf[n], env[n]), n
    if golden:
        assert H.rel_err(ref, torch.from_numpy(g[f"{golden}/encode"])) < 2e-5
    # decoder, with quantisation and without
    for nq in (False, True):
        plan = oc.ae_decode_plan(asd, ap, force_not_quantize=nq)
        names = [s.name for s in plan]
        assert len(set(names)) == len(names) and names[-1] == "dec.head", names
        assert names[:3] == (["dec.pq", "dec.in", "dec.mid.block_1"] if nq else ["dec.idx", "dec.zq", "dec.pq"]), names
        env = oc.run_plan(plan, {"z": z})
        ref, ridx = _straight_decode(asd, ap, z, force_not_quantize=nq)
        got, gidx = oc.vq_decode(asd, ap, z, force_not_quantize=nq, return_indices=True)
        assert torch.equal(env["dec.head"], ref) and torch.equal(got, ref) and torch.equal(oc.vq_decode(asd, ap, z, force_not_quantize=nq), ref)
        if nq:
            assert gidx is None and ridx is None
        else:
            assert torch.equal(env["dec.idx"], ridx) and torch.equal(gidx, ridx)
            zq, qidx = oc.vq_quantize(asd, z)
            assert torch.equal(zq, env["dec.zq"]) and torch.equal(qidx, ridx)
        tf = _teacher_forced(plan, env)
        for n in names:
            assert torch.equal(tf[n], env[n]), n
        if golden and not nq:
            assert H.rel_err(ref, torch.from_numpy(g[f"{golden}/decode"])) < 2e-5
            assert np.array_equal(ridx.numpy().astype(np.int32), g[f"{golden}/decode_idx"])


@pytest.mark.parametrize("tag", ["tiny_fe8", "realsr"])
def test_plans_in_float64(tag):
    """float64 weights and inputs keep every step in float64 (GroupNorm included), and the result agrees with the fp32 oracle to fp32
    round-off"""
    ap, asd, img, z, _ = _inputs(tag)
    sd64 = {k: v.double() for k, v in asd.items()}
    worst = 0.0
    for plan64, plan32, inp in ((oc.ae_encode_plan(sd64, ap), oc.ae_encode_plan(asd, ap), {"x": img}),
                                (oc.ae_decode_plan(sd64, ap), oc.ae_decode_plan(asd, ap), {"z": z}),
                                (oc.ae_decode_plan(sd64, ap, True), oc.ae_decode_plan(asd, ap, True), {"z": z})):
        env64 = oc.run_plan(plan64, {k: v.double() for k, v in inp.items()})
        env32 = oc.run_plan(plan32, dict(inp))
        for s in plan64:
            a, b = env64[s.name], env32[s.name]
            if s.name == "dec.idx":
                assert a.dtype == torch.int64 and (a != b).float().mean().item() <= 1e-3
                continue
            assert a.dtype == torch.float64, (s.name, a.dtype)
            if s.name == "dec.zq" and not torch.equal(env64["dec.idx"], env32["dec.idx"]):
                continue   # (a tie broken differently: another codebook row)
            e = ((a - b.double()).abs().max() / a.abs().max()).item()
            worst = max(worst, e)
            assert e < 2e-5, (s.name, e)
        # really float64 arithmetic, not float32 values in a float64 container: the result does not round-trip through float32
        out = env64[plan64[-1].name]
        assert (out.float().double() != out).float().mean().item() > 0.9
    assert worst > 0.0
    print(f"{tag}: float64 plans vs fp32 oracle, worst step {worst:.2e}")


@pytest.mark.parametrize("key,B,h,w", [("realsr", 32, 64, 64), ("realsr", 3, 64, 64), ("realsr", 2, 40, 24), ("faceir", 16, 64, 64),
                                       ("realsr", 1, 64, 128)])
def test_fp32_oracle_argmin_meets_the_cap_against_float64(key, B, h, w):
    """The GPU test lets an index differ from the float64 argmin where the float64 distances are within a few fp32 roundings of each other,
    but caps the share of differing positions at 0.1 % per image.  On the very latents it uses, the fp32 CPU oracle - the reference's own
    arithmetic - meets that cap against float64, so the cap asks nothing of the engine that the reference does not deliver."""
    ap = to_plain(load_config(CONFIGS[key]))["autoencoder"]["params"]
    asd = H.synth.synthetic_state_dict(ae_param_spec(ap), H.SEED_W)
    z = H.vq_latents(B, int(ap["embed_dim"]), h, w, 2000 + B)
    idx = torch.argmin(oc.vq_distances(asd, z), dim=1).view(B, -1)
    e64 = asd["quantize.embedding.weight"].double()
    worst = 0.0
    for b in range(B):
        differ, bad, _ = H.vq_check(z[b:b + 1].double(), e64, idx[b])
        worst = max(worst, differ)
        assert bad == 0 and differ <= H.VQ_CAP, (b, differ, bad)
    print(f"{key} B={B} {h}x{w}: fp32 oracle vs float64 argmin, worst share of differing positions per image {worst:.2e}")


@pytest.mark.parametrize("regime", R.REGIMES)
def test_regime_is_what_it_claims_and_its_yardstick_is_small(regime):
    """The regime cases of tests/test_ae_blocks_gpu.py (realsr, B = 1: encode 256 x 256, decode a 40 x 24 latent), oracle only.  quiet: the
    median GroupNorm variance within 100 eps (the minimum far below eps); loud: both attention softmaxes peaked, conv outputs well inside
    fp16; every regime finite and centred enough that GroupNorm's E[x^2] - mean^2 in fp32 costs ~1e-6 at most (|mean| / std <= 4 over
    every group).  The tolerance's yardstick, the float32 oracle's own error on each teacher-forced block, stays <= 1e-4.  (The
    autoencoder has no zero_module tensors: zero_init is the synthetic draw again, at this batch and these shapes.)"""
    up, ap, dp = H.realsr_params()
    _, asd = H.weights(up, ap)
    sd = R.regime_sd(asd, regime)
    if regime == "zero_init":
        assert H.synth.zero_module_names(asd.keys()) == [] and all(torch.equal(sd[k], asd[k]) for k in asd)
    assert torch.equal(sd["quantize.embedding.weight"], asd["quantize.embedding.weight"])
    if regime == "quiet":
        assert all(torch.equal(sd[k], asd[k]) for k in asd if k.startswith(("quant_conv.", "post_quant_conv.")))
        assert torch.equal(sd["decoder.conv_in.weight"], asd["decoder.conv_in.weight"] * 0.01)
    sd64 = {k: v.double() for k, v in sd.items()}
    x, z = R.ae_case_inputs(ap, "encode", 1, 256, 256), R.ae_case_inputs(ap, "decode", 1, 40, 24)
    var_eps = []
    for call, plan64, plan32, inp in (("encode", oc.ae_encode_plan(sd64, ap), oc.ae_encode_plan(sd, ap), {"x": x.double()}),
                                      ("decode", oc.ae_decode_plan(sd64, ap), oc.ae_decode_plan(sd, ap), {"z": z.double()})):
        with R.probe() as p:
            env = oc.run_plan(plan64, inp)
        var_eps += p.var_eps
        print(f"\n{regime} {call}: GroupNorm var / eps median {p.median_var_eps():.3g} minimum {p.min_var_eps():.3g}, max |mean| / std "
              f"{p.max_offcentre():.2f}, median largest probability {p.median_pmax():.3f}, largest |conv output| {p.conv:.3g}")
        assert p.finite and all(bool(torch.isfinite(env[s.name]).all()) for s in plan64 if s.name != "dec.idx")
        assert p.max_offcentre() <= 4.0
        if regime == "loud":
            assert p.median_pmax() >= 0.5 and p.conv <= 1000.0
        worst = (0.0, "-")
        for s64, s32 in zip(plan64, plan32):
            if s64.name in ("dec.idx", "dec.zq"):
                continue
            e = max(R.err32(s32, [env[i] for i in s64.inputs], env[s64.name]))
            worst = max(worst, (e, s64.name))
            assert e <= R.ERR32_CAP, (s64.name, e)
        print(f"{regime} {call}: float32 oracle against float64, teacher-forced, worst block {worst[0]:.3e} ({worst[1]})")
    if regime == "quiet":
        assert torch.cat(var_eps).median().item() <= 100.0


def _plan_dims(cname, call, B, Hh, Ww):
    """name -> (B, C, H, W) of every traced step of the plan (fp32 oracle at batch 1, synthetic weights)"""
    ap = to_plain(load_config(cname))["autoencoder"]["params"]
    asd = H.synth.synthetic_state_dict(ae_param_spec(ap), H.SEED_W)
    g = torch.Generator().manual_seed(5)
    if call == "encode":
        plan, env = oc.ae_encode_plan(asd, ap), {"x": torch.rand(1, 3, Hh, Ww, generator=g) * 2 - 1}
    else:
        plan, env = oc.ae_decode_plan(asd, ap, call == "decode_nq"), {"z": torch.randn(1, int(ap["embed_dim"]), Hh, Ww, generator=g) * 0.7}
    env = oc.run_plan(plan, env)
    return {s.name: (B,) + tuple(env[s.name].shape[1:]) for s in plan if s.name not in ("enc.z", "dec.idx", "dec.head")}


FAKE = [("realsr", "encode", 32, 256, 256, 2), ("realsr", "encode", 32, 256, 256, 0), ("realsr", "decode", 32, 64, 64, 0),
        ("realsr", "decode", 32, 64, 64, 2), ("realsr", "decode", 32, 64, 64, 1), ("realsr", "encode", 3, 256, 256, 2),
        ("realsr", "decode", 3, 64, 64, 0), ("realsr", "decode", 2, 40, 24, 0), ("realsr", "decode_nq", 2, 64, 64, 0),
        ("faceir", "encode", 16, 512, 512, 2), ("faceir", "decode", 16, 64, 64, 0),
        # the tile pool's size classes and batch 1 (the rows tests/test_ae_blocks_gpu.py adds to the square bench shapes)
        ("realsr", "encode", 1, 256, 512, 2), ("realsr", "decode", 1, 64, 128, 0), ("realsr", "decode", 6, 128, 64, 0),
        ("realsr", "decode", 1, 128, 128, 0), ("realsr", "decode", 1, 64, 128, 2)]


@pytest.mark.parametrize("key,call,B,Hh,Ww,prec", FAKE, ids=[f"{k}-{c}-B{b}-{h}x{w}-p{p}" for k, c, b, h, w, p in FAKE])
def test_trace_names_are_the_plan_blocks_without_a_gpu(key, call, B, Hh, Ww, prec):
    """RS_FAKE_DEVICE=1 (test-hooks library, see _fake_device_plumbing.py): a traced rs_vq_encode / rs_vq_decode records every block of
    the plan exactly once, with the plan's dims, plus inner records under a block's prefix; and tracing leaves the pass alone - the same
    launch count, pool, tickets and sequence numbers as the untraced call."""
    from resshift_amd import build as _b

    cname = CONFIGS[key]
    env = dict(os.environ, RS_FAKE_DEVICE="1", RESSHIFT_HIP_LIB=_b.build_testhooks(), **NO_GPU)
    r = subprocess.run([sys.executable, os.path.join(H.ROOT, "tests", "_fake_device_ae_trace.py"), cname, call, str(B), str(Hh), str(Ww), str(prec)],
                       env=env, capture_output=True, text=True, timeout=600)
    fake = re.findall(r"\[fake device\] (dry: .*)", r.stderr)
    calls = re.findall(r"CALL (\w+) rc -?\d+ launches (\d+) records (\d+)", r.stdout)
    assert len(fake) == 2 and len(calls) == 2, (r.stdout[-800:], r.stderr[-1500:])
    assert fake[0] == fake[1], fake                                  # dry / real bookkeeping of the two calls
    assert calls[0][1] == calls[1][1] and int(calls[0][2]) == 0, calls   # network launches; no records untraced
    recs = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("REC ")]
    assert len(recs) == int(calls[1][2]) and recs, calls
    names = [n for n, *_ in recs]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    dims = _plan_dims(cname, call, B, Hh, Ww)
    blocks = {n: tuple(int(v) for v in d) for n, *d in recs if n in dims}
    assert set(blocks) == set(dims), (sorted(set(dims) - set(blocks)), sorted(set(blocks) - set(dims)))
    for n, d in dims.items():
        assert blocks[n] == d, (n, blocks[n], d)
    # every other record is an inner one, named under the prefix of a block of the plan
    for n in names:
        if n not in dims:
            parts = n.split(".")
            assert any(".".join(parts[:k]) in dims for k in range(1, len(parts))), n
    print(f"{key} {call} B={B} p{prec}: {len(dims)} plan blocks, {len(names)} records, {calls[1][1]} launches traced and untraced")

"""The engine on network structures off the two the rest of the suite builds (oracle/cases.py: STRUCTURES; tests/_structures.py: the cases):
every UNet and autoencoder block against float64, teacher-forced, per image, and the whole loop of two pairs against the oracle.

The comparison is that of tests/test_unet_blocks_gpu.py / tests/test_ae_blocks_gpu.py (their _pick, their check_blocks, their TOL): a
traced call (Engine.debug_enable) runs the same graph as an untraced one - asserted: same bits, same launch count - and records every
block boundary; each block of the oracle's plan is fed the engine's own recorded inputs in float64 and compared with the engine's output
of that block, max |engine - ref| / max |ref| per image.  Tolerance of a block and image: max(TOL[prec], k * err32), err32 the float32
oracle's own error on the same teacher-forced inputs against its float64 value (the reference's arithmetic, never the engine's), k = 4
for fp32 storage, k = 8 for split (tests/_regimes.py: K32); fp16 keeps TOL["fp16"].  tests/test_structures_cpu.py walks every case here on
the fake device first.  Run with -s for the kernel families of every case and the block nearest its tolerance.

Measured on the MI355X (51 cases, 17 s in all; the slowest, heads6_mc192 at B = 16 in split storage, 2.7 s - the float64 and float32 oracle
passes over 16 images).  Per structure and storage the block and image nearest its tolerance: error / err32.  k * err32 stayed under
TOL[prec] on every block of every structure, so TOL[prec] applied everywhere (split 5e-6, fp16 2.5e-3, fp32 1e-5) and no block needed
more - heads6_mc192's K = 9 x 768 sums included (out.1: 3.0e-6 in fp32 storage, err32 2.7e-7).

  structure      case        split                          fp16                 fp32
  one_level      B3 16x16    5.0e-7 / 2.4e-7 head           7.9e-4 out.1         6.0e-7 / 3.1e-7 in.1.res
  three_uneven   B3 32x32    6.0e-7 / 3.2e-7 head           9.0e-4 out.4         7.0e-7 / 3.9e-7 in.3
  three_uneven   B2 64x32    6.1e-7 / 3.0e-7 head
  mult0          B3 16x16    5.5e-7 / 3.1e-7 head           7.2e-4 out.3         8.2e-7 / 2.3e-7 head
  depth3         B3 32x32    5.0e-7 / 3.4e-7 head           1.4e-3 out.0         7.4e-7 / 3.4e-7 in.2
  no_level_attn  B3 16x16    9.2e-7 / 3.0e-7 head           1.0e-3 mid.swin      7.4e-7 / 3.5e-7 head
  fe1_mask       B3 16x16    7.2e-7 / 3.9e-7 in.0           1.2e-3 mid.swin      8.7e-7 / 3.9e-7 in.2
  heads6_mc128   B16 32x32   1.5e-6 / 2.7e-7 head           9.1e-4 in.1          2.9e-6 / 2.8e-7 out.1
  heads6_mc128   B2 32x32    1.4e-6 / 3.4e-7 head
  heads6_mc192   B16 32x32   1.9e-6 / 2.4e-7 head           9.6e-4 mid.swin      3.0e-6 / 2.7e-7 out.1
  heads6_mc192   B2 32x32    1.4e-6 / 3.2e-7 head
  ae_f1          encode      6.8e-7 / 3.1e-7 enc.out        4.6e-4 enc.mid.block_1      5.8e-7 / 3.3e-7 enc.out
  ae_f1          decode      8.0e-7 / 4.3e-7 dec.head       5.7e-4 dec.mid.block_1      5.7e-7 / 2.8e-7 dec.mid.block_2
  ae_f8_equal    encode      4.1e-7 / 2.4e-7 enc.out        6.1e-4 enc.down.2.block.0   6.7e-7 / 4.0e-7 enc.down.0.ds
  ae_f8_equal    decode      6.8e-7 / 3.8e-7 dec.head       7.0e-4 dec.mid.attn         8.1e-7 / 3.9e-7 dec.head
  ae_f2_wide     encode      1.1e-6 / 2.5e-7 enc.out        5.8e-4 enc.down.0.block.0   1.2e-6 / 2.5e-7 enc.out
  ae_f2_wide     decode      1.1e-6 / 3.8e-7 dec.head       5.6e-4 dec.up.0.block.0     7.7e-7 / 2.4e-7 dec.head

VQ (ae_f8_equal: the D = 4 search over 256 codes, 256 positions per image): no position differs from the float64 argmin in any storage.
Loops (latent error, VQ agreement, image dB): one_level + ae_f1 split 1.1e-6 / 1.0 / 142, fp32 1.5e-6 / 1.0 / 139, fp16 2.1e-3 / 0.990 / 54;
fe1_mask + ae_f8_equal split 4.2e-6 / 1.0 / 138, fp32 3.6e-6 / 1.0 / 135, fp16 5.2e-3 / 0.988 / 40.
Kernel families: every small structure runs the implicit-GEMM family of its storage alone (no plane here reaches the halo or Winograd
kernels); heads6_mc128 / heads6_mc192 add the fused attention (10 launches) in fp16 and split storage at both batches and the fused MLP
(4 launches, every one ending in E = 192 channels: no patch-unembed fold) at B = 16; their fp32 passes run the exact implicit GEMM alone.
"""
import numpy as np
import pytest
import torch

import _regimes as R
import _structures as T
import helpers as H
from oracle import cases, resshift_oracle as oc
from resshift_amd.engine import Engine, parse_precision
from test_ae_blocks_gpu import TOL as TOL_AE, check_blocks
from test_unet_blocks_gpu import TOL, _pick, _worse

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
S = T.S
assert TOL_AE == TOL
F_ATTN, F_MLP, F_ATTN_S, F_MLP_S = 5, 6, 7, 8   # Engine.FAMILIES: the fused qkv + window attention + proj and the fused Swin MLP, fp16 / split storage
assert all(("win_attn_qkv" in Engine.FAMILIES[a]) and ("swin_mlp" in Engine.FAMILIES[m]) for a, m in ((F_ATTN, F_MLP), (F_ATTN_S, F_MLP_S)))
STEPS = int(cases.TINY_DIFFUSION["steps"])

_unets, _aes, _loops = {}, {}, {}
_margin = {}   # (structure, what, prec) -> (error, block, err32, tolerance) of the block and image nearest its tolerance


@pytest.fixture(scope="module", autouse=True)
def _table():
    """after the module: per structure, case and storage the block nearest its tolerance (-s)"""
    yield
    if _margin:
        print("\nblock nearest its tolerance per structure, case and storage: error, the float32 oracle's error there (err32), tolerance applied")
        for (tag, what, prec), (e, name, e32, tol) in _margin.items():
            print(f"{tag:<14}{what:<12}{prec:<6}{e:>11.3e} {name:<18}{e32:>11.3e}{tol:>11.3e}")
    _unets.clear(), _aes.clear(), _loops.clear()


def _usable(eng_call, prec):
    """run `eng_call(prec)`; where the structure's weights cannot take the storage the engine says so, and the case falls back to fp32"""
    try:
        return eng_call(parse_precision(prec)), prec
    except RuntimeError as err:
        assert prec != "fp32" and ("fp16 range" in str(err) or "split precision" in str(err)), err
        return eng_call(parse_precision("fp32")), "fp32"


def _unet(tag, gpu):
    if tag not in _unets:
        up = S["unet"][tag]
        usd = T.unet_weights(up)
        eng = Engine(unet_params=up, ae_params=None, device=gpu)
        eng.load_state_dicts(unet_sd=usd)
        eng.mark_weights_ready()
        _unets[tag] = (up, usd, T.double(usd), eng)
    return _unets[tag]


def _uid(tag, B, h, w, prec):
    return f"{tag}-B{B}-" + (f"{h}x{w}-" if h else "") + prec


@pytest.mark.parametrize("tag,B,h,w,prec", T.UNET, ids=[_uid(*c) for c in T.UNET])
def test_every_unet_block_of_a_structure_against_float64(gpu, tag, B, h, w, prec):
    up, usd, sd64, eng = _unet(tag, gpu)
    hz = int(up["image_size"])
    h, w = (h, w) if h else (hz, hz)
    x, lq, mask, t = R.unet_case_inputs(up, B, h, w, STEPS, "mixed")
    assert len(set(t)) > 1
    dev = dict(lq=lq.to(gpu), mask=mask.to(gpu) if mask is not None else None)
    with_mask = mask is not None
    plan = oc.unet_plan(sd64, up, with_lq=True, with_mask=with_mask)

    # the same pass untraced and traced: same bits, same network launches
    eng.debug_enable(False)
    out, prec = _usable(lambda p: eng.unet_forward(x.to(gpu), t, prec=p, **dev), prec)
    torch.cuda.synchronize()
    n_plain = eng.last_launch_count()
    pick = _pick(B, h, w)
    eng.debug_enable(True)
    try:
        out_tr = eng.unet_forward(x.to(gpu), t, prec=parse_precision(prec), **dev)
        n_traced = eng.last_launch_count()
        fam = [n for name, fl, ms, n in eng.profile_families()]
        trace = {k: v.double().cpu() for k, v in eng.debug_trace(names=[s.name for s in plan], images=pick).items()}
    finally:
        eng.debug_enable(False)
    assert torch.equal(out, out_tr), "a traced pass computes something else than an untraced one"
    assert n_plain == n_traced, (n_plain, n_traced)
    print(f"\n{_uid(tag, B, h, w, prec)}: {n_traced} launches, families " + ", ".join(f"{Engine.FAMILIES[k].split(' (')[0]} x {n}" for k, n in enumerate(fam) if n))

    # the kernel families the structure is there for
    fused = [fam[F_ATTN], fam[F_MLP], fam[F_ATTN_S], fam[F_MLP_S]]
    if tag in ("depth3", "mult0"):   # 3 heads of E = 96 / 2 heads of E = 64: no fused Swin kernel exists for them
        assert fused == [0, 0, 0, 0], fam
    if tag in T.BIG and prec != "fp32":
        k_attn, k_mlp = (F_ATTN, F_MLP) if prec == "fp16" else (F_ATTN_S, F_MLP_S)
        assert fam[k_attn] == 10, fam   # every Swin block of the five layers
        assert fam[k_mlp] == (4 if B == T.B_FUSED else 0), fam   # the 32 x 32 level's two layers once they have 16384 tokens
        if B == T.B_FUSED:
            # ... and once more with the profiler's brackets, for the launch shapes: still the same bits.  Every fused MLP launch ends in E
            # channels (patch_unembed is not folded into it: that form exists for 160 channels only) and patch_unembed runs as a 1x1 conv
            # launch of its own, [M, C] with K = E
            eng.profile_enable(True)
            try:
                out_pr = eng.unet_forward(x.to(gpu), t, prec=parse_precision(prec), **dev)
                torch.cuda.synchronize()
                shapes, _ = eng.profile_shapes()
            finally:
                eng.profile_enable(False)
            assert torch.equal(out, out_pr)
            E, C, M = int(up["swin_embed_dim"]), int(up["model_channels"]), B * h * w
            mlp = [s for s in shapes if s["family"] == k_mlp]
            assert mlp and all((s["M"], s["N"], s["K"]) == (M, E, 4 * E) for s in mlp) and sum(s["launches"] for s in mlp) == 4, mlp
            n_un = sum(s["launches"] for s in shapes if s["family"] not in (k_attn, k_mlp) and (s["M"], s["N"], s["K"]) == (M, C, E))
            assert n_un == (2 if C != E else 4), (n_un, shapes)   # (C = E: patch_embed has the same shape)

    # every block of the plan, teacher-forced, in float64, per image
    host = {"x": x[pick].double(), "t": torch.tensor([t[b] for b in pick]), "lq": lq[pick].double()}
    if with_mask:
        host["mask"] = mask[pick].double()
    k32 = R.K32.get(prec)
    plan32 = {s.name: s for s in oc.unet_plan(usd, up, with_lq=True, with_mask=with_mask)} if k32 else None
    got_head = out[pick].double().cpu()
    env = dict(host)
    failures, missing, own = [], [], (0.0, "-", float("nan"), TOL[prec])
    for s in plan:
        if s.name not in ("emb", "head") and s.name not in trace:
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
        for k, b in enumerate(pick):
            e = ((got[k] - ref[k]).abs().max() / ref[k].abs().max().clamp_min(1e-30)).item()
            tol = max(TOL[prec], k32 * e32[k]) if k32 else TOL[prec]
            if _worse(e / tol, own[0] / own[3]):
                own = (e, s.name, e32[k] if k32 else float("nan"), tol)
            if not np.isfinite(e) or e > tol:
                failures.append(f"{s.name}: image {b} (t={t[b]}) error {e:.3e} > {tol:.1e}" + (f" (err32 {e32[k]:.3e})" if k32 else ""))
    _margin[(tag, f"B{B} {h}x{w}", prec)] = own
    print(f"{len(plan) - 1} blocks x {len(pick)} images; block nearest its tolerance {own[1]}: error {own[0]:.3e}, err32 {own[2]:.3e}, tolerance {own[3]:.3e}")
    assert not missing, f"blocks of the plan missing from the trace: {missing}"
    assert not failures, "\n".join(failures[:40])


def _ae(tag, gpu):
    if tag not in _aes:
        ap = S["ae"][tag]
        asd = T.ae_weights(ap)
        eng = Engine(unet_params=None, ae_params=ap, device=gpu)
        eng.load_state_dicts(ae_sd=asd)
        eng.mark_weights_ready()
        _aes[tag] = (ap, asd, T.double(asd), eng)
    return _aes[tag]


@pytest.mark.parametrize("tag,call,B,prec", T.AE, ids=["-".join(str(v) for v in c) for c in T.AE])
def test_every_autoencoder_block_of_a_structure_against_float64(gpu, tag, call, B, prec):
    ap, asd, sd64, eng = _ae(tag, gpu)
    h, w = T.ae_plane(tag, call)
    x = R.ae_case_inputs(ap, call, B, h, w)   # (decode: helpers.vq_latents)
    if call == "encode":
        plan, hname = oc.ae_encode_plan(sd64, ap), "x"
        run = lambda p: (eng.vq_encode(x.to(gpu), prec=p), None)
    else:
        plan, hname = oc.ae_decode_plan(sd64, ap), "z"
        run = lambda p: eng.vq_decode(x.to(gpu), prec=p, return_indices=True)
    pick = list(range(B))
    want = [s.name for s in plan] + ["dec.zq.z"]

    eng.debug_enable(False)
    (out, idx), prec = _usable(run, prec)
    torch.cuda.synchronize()
    n_plain = eng.last_launch_count()
    eng.debug_enable(True)
    try:
        out_tr, idx_tr = run(parse_precision(prec))
        n_traced = eng.last_launch_count()
        fam = [n for name, fl, ms, n in eng.profile_families()]
        trace = {k: v.cpu() for k, v in eng.debug_trace(names=want, images=pick).items()}
    finally:
        eng.debug_enable(False)
    assert torch.equal(out, out_tr) and (idx is None or torch.equal(idx, idx_tr)), "a traced pass computes something else than an untraced one"
    assert n_plain == n_traced, (n_plain, n_traced)
    print(f"\n{tag} {call} B={B} {h}x{w} {prec}: {n_traced} launches, families " + ", ".join(f"{Engine.FAMILIES[k].split(' (')[0]} x {n}" for k, n in enumerate(fam) if n))

    k32, margin, own = R.K32.get(prec), [], {}
    plan32 = {s.name: s for s in (oc.ae_encode_plan(asd, ap) if call == "encode" else oc.ae_decode_plan(asd, ap))} if k32 else None
    idx_p = idx.view(B, -1).cpu() if call == "decode" else None
    failures, missing = check_blocks(plan, {hname: x}, trace, out.cpu(), idx_p, asd, sd64, pick, prec, TOL[prec], own, plan32, k32, margin)
    _margin[(tag, call, prec)] = margin[0]
    print(f"{len(plan)} blocks x {B} images; block nearest its tolerance {margin[0][1]}: error {margin[0][0]:.3e}, err32 {margin[0][2]:.3e}, "
          f"tolerance {margin[0][3]:.3e}; VQ positions differing from the float64 argmin {own.get(('dec.idx (differ)', prec), 0.0):.2e}")
    assert not missing, f"blocks of the plan missing from the trace: {missing}"
    assert not failures, "\n".join(failures[:40])


def _loop(tag):
    """the oracle's loop of a pair, once"""
    if tag not in _loops:
        from oracle import make_golden_structures as ms

        up, ap, dp, with_mask = cases.structure_pair(tag)
        usd, asd = T.unet_weights(up), T.ae_weights(ap)
        y, noises, mask = ms.pair_inputs(tag)
        ref, aux = oc.sample_loop(usd, up, asd, ap, dp, y, noises, mask=mask, return_aux=True)
        _loops[tag] = (up, ap, dp, usd, asd, y, noises, mask, ref, aux)
    return _loops[tag]


@pytest.mark.parametrize("tag,B,prec", T.PAIRS, ids=["-".join(str(v) for v in c) for c in T.PAIRS])
def test_sample_loop_of_a_pair_vs_oracle(gpu, tag, B, prec):
    """the fused native loop against the oracle's with injected noise: the bounds of tests/test_engine_gpu.py: test_sample_loop_vs_oracle"""
    from resshift_amd import UNetModelSwin, VQModelTorch, create_gaussian_diffusion

    up, ap, dp, usd, asd, y, noises, mask, ref, aux = _loop(tag)
    assert y.shape[0] == B
    um = UNetModelSwin(**up).to(gpu)
    um.load_state_dict(usd, strict=True)
    am = VQModelTorch(**ap).to(gpu)
    am.load_state_dict(asd, strict=True)
    d = create_gaussian_diffusion(**dp)
    d.set_precision(prec, prec, prec)
    kw = {"lq": y.to(gpu)}
    if mask is not None:
        kw["mask"] = mask.to(gpu)
    out, gaux = d.p_sample_loop(y.to(gpu), um.eval(), first_stage_model=am.eval(), noise=noises[0].to(gpu), clip_denoised=False, model_kwargs=kw,
                                step_noises=[n.to(gpu) for n in noises[1:]], return_aux=True)
    torch.cuda.synchronize()
    zerr = H.rel_err(gaux["z_final"], aux["z_final"])
    agree = (gaux["indices"].cpu().long().reshape(-1) == aux["indices"].reshape(-1)).float().mean().item()
    p = H.psnr(out.cpu().clamp(-1, 1), ref.clamp(-1, 1))
    print(f"\nsample {tag} {prec}: latent rel err {zerr:.3e}, VQ agreement {agree:.4f}, image PSNR {p:.1f} dB")
    assert out.shape == ref.shape
    assert zerr < (2e-2 if prec == "fp16" else 5e-5)
    if prec != "fp16":
        assert agree >= 0.99 and p >= 60.0
    if prec == "fp32":
        g = T.fixture()
        assert H.psnr(out.cpu().clamp(-1, 1), torch.from_numpy(g[f"pair/{tag}/sample"].astype(np.float32)).clamp(-1, 1)) >= 60.0

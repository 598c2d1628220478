"""Per-request seeds on the GPU.  The reference of every value is the float64 restatement in tests/_philox_ref.py.

  * rs_noise_fill against the restatement rounded to fp32 (absolute 1e-5: u1, u2 and the sincospif argument are exact, so the error is
    that of logf, sqrtf, sincospif and two multiplies - a few ulp each, times r <= 5.77, below 4e-6 even at 10 ulp in total - while an
    indexing or counter mistake is O(1));
  * the seeded entry points are, bit for bit and launch for launch, the tensor entry points fed with rs_noise_fill's output;
  * the seeded schedulers equal the default ones fed those tensors, and a request's bits do not depend on the submit order;
  * end to end: the CPU oracle's loop fed the restatement's normals against p_sample_loop(seeds=).
"""
import ctypes

import numpy as np
import pytest
import torch

import helpers as H
import _philox_ref as P
from oracle import resshift_oracle as oc

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

_SHELLS, _REALSR, _SAMPLERS = {}, {}, {}
PRECS = ["fp16", "split", "fp32"]


def _shells(tag, dev):
    from resshift_amd import UNetModelSwin, VQModelTorch

    if tag not in _SHELLS:
        up, ap, _, _ = H.CASES[tag]
        usd, asd = H.weights(up, ap)
        um = UNetModelSwin(**up).to(dev)
        um.load_state_dict(usd, strict=True)
        am = VQModelTorch(**ap).to(dev)
        am.load_state_dict(asd, strict=True)
        _SHELLS[tag] = (um.eval(), am.eval(), usd, asd)
    return _SHELLS[tag]


def _realsr(dev):
    """the one realsr-sized model pair (and engine) of this file"""
    from resshift_amd import UNetModelSwin, VQModelTorch, create_gaussian_diffusion

    if "eng" not in _REALSR:
        up, ap, dp = H.realsr_params()
        usd, asd = H.weights(up, ap)
        um = UNetModelSwin(**up).to(dev)
        um.load_state_dict(usd, strict=True)
        am = VQModelTorch(**ap).to(dev)
        am.load_state_dict(asd, strict=True)
        d = create_gaussian_diffusion(**dp)
        _REALSR.update(um=um.eval(), am=am.eval(), d=d, eng=d._fused_engine(um, am), up=up, ap=ap, dp=dp, usd=usd, asd=asd)
    return _REALSR


def _sampler(tag, precision, chop_size=16, chop_stride=12, chop_bs=1, offset=16):
    from resshift_amd import ResShiftSampler
    from resshift_amd.config import ConfigNode

    up, ap, dp, _ = H.CASES[tag]
    if (tag, precision) not in _SAMPLERS:
        usd, asd = H.weights(up, ap)
        cfg = ConfigNode(model=ConfigNode(target="models.unet.UNetModelSwin", ckpt_path=None, params=up),
                         diffusion=ConfigNode(target="models.script_util.create_gaussian_diffusion", params=dp),
                         autoencoder=ConfigNode(target="ldm.models.autoencoder.VQModelTorch", ckpt_path=None, params=ap))
        _SAMPLERS[(tag, precision)] = (ResShiftSampler(cfg, sf=dp["sf"], seed=1, precision=precision,
                                                       state_dicts={"model": usd, "autoencoder": asd}), usd, asd)
    s, usd, asd = _SAMPLERS[(tag, precision)]
    s.chop_size, s.chop_stride, s.chop_bs, s.padding_offset = chop_size, chop_stride, chop_bs, offset
    return s, usd, asd


def _keys(B, base=4000):
    """distinct seeds (some above 2^32, one above 2^63) and streams"""
    return [(base + 7919 * b + (2 ** 40 if b % 3 == 1 else 0) + (2 ** 63 if b % 5 == 4 else 0), (b * 2654435761) % 2 ** 32 if b % 2 else b) for b in range(B)]


# ---------------------------------------------------------------------------------------------------------------- the generator
@pytest.mark.parametrize("per", [1, 3, 4, 5, 12288, 12289])
def test_noise_fill_matches_the_float64_restatement(gpu, per):
    from resshift_amd import _lib

    lib, B = _lib.load(), 64
    keys = _keys(B)
    draws = [(b * 5) % 17 for b in range(B)]
    want = np.stack([P.normals(s, st, k, per) for (s, st), k in zip(keys, draws)]).astype(np.float32)
    karr, darr = _lib.noise_keys(keys), (ctypes.c_int * B)(*draws)
    worst = 0.0
    for offset in (0, 1):   # a 16-byte aligned output, and one offset by 4 bytes (the element-by-element path)
        buf = torch.full((B * per + 8,), float("nan"), device=gpu)
        assert buf.data_ptr() % 16 == 0
        out = buf[offset:offset + B * per]
        _lib.check(lib.rs_noise_fill(karr, darr, out.data_ptr(), per, B, _lib.current_stream_ptr()), "rs_noise_fill")
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(B, per)
        assert np.isnan(buf[offset + B * per:].cpu().numpy()).all() and (offset == 0 or np.isnan(buf[:offset].cpu().numpy()).all())
        err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        worst = max(worst, err)
        print(f"rs_noise_fill per_image_count {per}, output offset {4 * offset} B: max abs error {err:.3e} vs the restatement (fp32)")
        assert err <= 1e-5, (per, offset, err)
    assert np.abs(want).max() <= np.sqrt(48 * np.log(2)) and worst <= 1e-5


def test_engine_noise_fill_groups_and_shape(gpu):
    um, am, _, _ = _shells("tiny", gpu)
    from resshift_amd import create_gaussian_diffusion

    eng = create_gaussian_diffusion(**H.CASES["tiny"][2])._fused_engine(um, am)
    keys = _keys(70)
    full = eng.noise_fill(keys, list(range(70)), (3, 16, 16))
    part = eng.noise_fill(keys[64:], list(range(64, 70)), (3, 16, 16))
    torch.cuda.synchronize()
    assert tuple(full.shape) == (70, 3, 16, 16) and torch.equal(full[64:], part)
    want = P.normals(*keys[69], 69, 768).astype(np.float32).reshape(3, 16, 16)
    assert np.abs(full[69].cpu().numpy() - want).max() <= 1e-5


# ---------------------------------------------------------------------------------------------------------------- seeded == fill + tensor
def _step_pair(eng, x0, y, mask, ts, keys, tables, sf, T, prec):
    zs = tuple(x0.shape[1:])
    noise = eng.noise_fill(keys, [T - t for t in ts], zs)
    xa, xb = x0.clone(), x0.clone()
    pa, pb = torch.empty_like(x0), torch.empty_like(x0)
    eng.sample_step(xa, y, ts, noise, tables, sf, mask=mask, prec=prec, pred_xstart=pa)
    la = eng.last_launch_count()
    eng.sample_step(xb, y, ts, None, tables, sf, mask=mask, prec=prec, pred_xstart=pb, keys=keys)
    lb = eng.last_launch_count()
    torch.cuda.synchronize()
    assert la == lb > 0, (ts, la, lb)
    assert torch.equal(pa, pb), ts
    assert torch.equal(xa, xb), (ts, (xa - xb).abs().max().item())
    assert not torch.equal(xa, x0)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tag", list(H.CASES))
def test_seeded_step_and_begin_equal_noise_fill_plus_tensor_call(gpu, tag, prec):
    from resshift_amd import create_gaussian_diffusion

    up, ap, dp, with_mask = H.CASES[tag]
    um, am, _, _ = _shells(tag, gpu)
    d = create_gaussian_diffusion(**dp)
    eng = d._fused_engine(um, am)
    y, noises, mask = H.case_inputs(up, ap, dp, with_mask, B=3)
    y, mask = y.to(gpu), (mask.to(gpu) if with_mask else None)
    tables, T = d.step_tables(), d.num_timesteps
    keys = _keys(3, base=17)
    x0 = (noises[1] * 1.2).to(gpu).contiguous()
    for ts in ([2, 2, 2], [0, 0, 0], [T - 1, 0, 1], [0, T - 1, 0]):   # uniform (also at t = 0), mixed with images at t = 0
        _step_pair(eng, x0, y, mask, ts, keys, tables, d.sf, T, prec)
    prior = eng.noise_fill(keys, [0, 0, 0], tuple(x0.shape[1:]))
    xa = eng.sample_begin(y, prior, tables, d.sf, d.scale_factor, prec_encode=prec)
    la = eng.last_launch_count()
    xb = eng.sample_begin(y, None, tables, d.sf, d.scale_factor, prec_encode=prec, keys=keys)
    lb = eng.last_launch_count()
    torch.cuda.synchronize()
    assert la == lb > 0 and torch.equal(xa, xb)
    with pytest.raises(ValueError, match="not both"):
        eng.sample_begin(y, prior, tables, d.sf, d.scale_factor, prec_encode=prec, keys=keys)
    with pytest.raises(ValueError, match="3 images but 2 keys"):
        eng.sample_step(x0.clone(), y, [1, 1, 1], None, tables, d.sf, mask=mask, prec=prec, keys=keys[:2])
    with pytest.raises(RuntimeError, match="noise is NULL"):   # the tensor call keeps its own message
        eng.sample_step(x0.clone(), y, [1, 1, 1], None, tables, d.sf, mask=mask, prec=prec)


def test_realsr_seeded_step_equals_noise_fill_plus_tensor_step(gpu):
    """realsr B = 4 under split (the shapes of tests/test_continuous_gpu.py): per_image_count 12288, the 16-byte path"""
    r = _realsr(gpu)
    eng, d = r["eng"], r["d"]
    tables, T = d.step_tables(), d.num_timesteps
    g = torch.Generator().manual_seed(7)
    x0 = torch.randn(4, 3, 64, 64, generator=g).to(gpu)
    y = (torch.rand(4, 3, 64, 64, generator=g) * 2 - 1).to(gpu)
    keys = _keys(4, base=99)
    for ts in ([9, 9, 9, 9], [14, 0, 7, 3]):
        _step_pair(eng, x0, y, None, ts, keys, tables, d.sf, T, "split")
    prior = eng.noise_fill(keys, [0] * 4, (3, 64, 64))
    xa = eng.sample_begin(y, prior, tables, d.sf, d.scale_factor, prec_encode="split")
    la = eng.last_launch_count()
    xb = eng.sample_begin(y, None, tables, d.sf, d.scale_factor, prec_encode="split", keys=keys)
    torch.cuda.synchronize()
    assert la == eng.last_launch_count() and torch.equal(xa, xb)


@pytest.mark.parametrize("B", [3, 70])
def test_rs_sample_seeded_equals_rs_sample(gpu, B):
    """the whole loop in one call, B = 3 and B = 70 (> RS_MAX_ROWS: the keys travel through their device copy): image, final latent, VQ
    indices and launch count"""
    from resshift_amd import create_gaussian_diffusion

    up, ap, dp, _ = H.CASES["tiny"]
    um, am, _, _ = _shells("tiny", gpu)
    d = create_gaussian_diffusion(**dp)
    eng = d._fused_engine(um, am)
    tables, T = d.step_tables(), d.num_timesteps
    y = (torch.rand(B, 3, 16, 16, generator=torch.Generator().manual_seed(5)) * 2 - 1).to(gpu)
    keys = _keys(B, base=123)
    noise = torch.stack([eng.noise_fill(keys, [k] * B, (3, 16, 16)) for k in range(T + 1)])
    kw = dict(sf=d.sf, scale_factor=d.scale_factor, prec_unet="split", prec_encode="split", prec_decode="fp16", return_aux=True)
    ref, aux = eng.sample(y, noise, tables, **kw)
    la = eng.last_launch_count()
    got, gaux = eng.sample(y, None, tables, keys=keys, **kw)
    lb = eng.last_launch_count()
    torch.cuda.synchronize()
    assert la == lb > 0, (la, lb)
    assert torch.equal(gaux["z_final"], aux["z_final"]) and torch.equal(gaux["indices"], aux["indices"]) and torch.equal(got, ref)


# ---------------------------------------------------------------------------------------------------------------- schedulers
def _draws_of(eng, key, T, zs):
    """[T+1, *zs]: draws 0 .. T of one key, from rs_noise_fill"""
    return eng.noise_fill([key] * (T + 1), list(range(T + 1)), zs)


@pytest.mark.parametrize("prec", ["split", "fp16"])
def test_seeded_continuous_sampler_equals_default_one_fed_noise_fill(gpu, prec):
    """the staggered schedule of test_continuous_staggered_schedule_vs_oracle (max_batch 4, six requests arriving at steps 0, 0, 1, 3, 3, 5)"""
    from resshift_amd.continuous import ContinuousSampler

    up, ap, dp, _ = H.CASES["tiny"]
    s, _, _ = _sampler("tiny", prec)
    y, _, _ = H.case_inputs(up, ap, dp, False, B=6)
    y = y.to(gpu)
    keys = _keys(6, base=31)
    T = dp["steps"]
    arrivals = [0, 0, 1, 3, 3, 5]

    def run(seeded):
        cs = ContinuousSampler(s, max_batch=4, seeded=seeded)
        ids, out, k = {}, {}, 0
        while len(ids) < 6 or cs.pending():
            for r in [r for r in range(6) if arrivals[r] == k]:
                if seeded:
                    rid, = cs.submit(y[r:r + 1], seed=keys[r][0], stream=keys[r][1])
                else:
                    dr = _draws_of(s.engine, keys[r], T, (3, 16, 16))
                    rid, = cs.submit(y[r:r + 1], noise=dr[0:1], step_noises=[dr[j:j + 1] for j in range(1, T + 1)])
                ids[rid] = r
            out.update(cs.step())
            k += 1
        torch.cuda.synchronize()
        assert (cs._N is None) == seeded
        return {ids[rid]: img.clone() for rid, img in out.items()}

    a, b = run(True), run(False)
    assert sorted(a) == sorted(b) == list(range(6))
    for r in range(6):
        assert torch.equal(a[r], b[r]), (r, (a[r] - b[r]).abs().max().item())


def test_seeded_pool_is_independent_of_the_submit_order(gpu):
    from resshift_amd.continuous import ContinuousSampler

    up, ap, dp, _ = H.CASES["tiny"]
    s, _, _ = _sampler("tiny", "parity")
    y, _, _ = H.case_inputs(up, ap, dp, False, B=4)
    y = y.to(gpu)
    res = []
    for order in ([0, 1, 2, 3], [3, 1, 0, 2]):
        cs = ContinuousSampler(s, max_batch=4, seeded=True)
        ids = {cs.submit(y[r:r + 1], seed=1000 + r)[0]: r for r in order}
        out = cs.drain()
        torch.cuda.synchronize()
        res.append({ids[rid]: img.clone() for rid, img in out.items()})
    for r in range(4):
        assert torch.equal(res[0][r], res[1][r]), r
    assert not torch.equal(res[0][0], res[0][1])


def test_seeded_tile_pool_and_sample_tiled_equal_the_tensor_paths(gpu):
    """a mixed folder - 40 x 28 and 20 x 30 (class 32 x 32), 12 x 40 (class 16 x 32) at chop 32 / stride 24 - through a seeded TilePool and
    through the default one fed the rs_noise_fill tensors of the same (seed, tile index) keys; sample_tiled(seed=) against
    sample_tiled(tile_noises=) on the 40 x 28 image at chop 16 / stride 12 / chop_bs 2"""
    from resshift_amd.tilepool import TilePool, class_key, tile_windows

    _, _, dp, _ = H.CASES["tiny"]
    T = dp["steps"]
    s, _, _ = _sampler("tiny", "parity", 32, 24, 1, 16)
    g = torch.Generator().manual_seed(61)
    sizes = [(40, 28), (20, 30), (12, 40)]
    ims = [(torch.rand(3, h, w, generator=g) * 2 - 1).to(gpu) for h, w in sizes]
    seeds = [70001, 2 ** 45 + 3, 70003]
    classes = set()

    def tile_noises(h, w, seed, chop, stride):
        wins = tile_windows(h, w, chop, stride)
        key = class_key(wins[0][2], wins[0][3], 16)
        classes.add(key)
        out = []
        for j in range(len(wins)):
            dr = _draws_of(s.engine, (seed, j), T, (3, key[0], key[1]))
            out.append((dr[0:1], [dr[k:k + 1] for k in range(1, T + 1)]))
        return out

    def run(seeded):
        tp = TilePool(s, max_batch=4, seeded=seeded, keep_log=True)
        ids = {}
        for i, im in enumerate(ims):
            rid = tp.submit(im, seed=seeds[i]) if seeded else tp.submit(im, tile_noises=tile_noises(*sizes[i], seeds[i], 32, 24))
            ids[rid] = i
        out = tp.drain()
        torch.cuda.synchronize()
        assert any(len({i for i, _ in b}) > 1 for b in tp.batches)   # tiles of two images shared an engine step
        return {ids[rid]: img.clone() for rid, img in out.items()}

    a, b = run(True), run(False)
    assert len(classes) == 2
    for i in range(3):
        assert tuple(a[i].shape) == (3, sizes[i][0] * 4, sizes[i][1] * 4)
        assert torch.equal(a[i], b[i]), (i, (a[i] - b[i]).abs().max().item())
    # sample_tiled: six tiles, two per sampler call
    s, _, _ = _sampler("tiny", "parity", 16, 12, 2, 16)
    per_tile = tile_noises(40, 28, 555, 16, 12)
    assert len(per_tile) == 6
    calls = [(torch.cat([per_tile[2 * k][0], per_tile[2 * k + 1][0]]), [torch.cat([per_tile[2 * k][1][j], per_tile[2 * k + 1][1][j]]) for j in range(T)])
             for k in range(3)]
    ref = s.sample_tiled(ims[0][None], tile_noises=calls)
    got = s.sample_tiled(ims[0][None], seed=555)
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    # ... and the seeded pool gives that image the same tiles' noise (one batch of six on both sides: bit for bit)
    s.chop_bs = 6
    ref6 = s.sample_tiled(ims[0][None], seed=555)
    tp = TilePool(s, max_batch=6, seeded=True)
    rid = tp.submit(ims[0], seed=555)
    out = tp.drain()
    torch.cuda.synchronize()
    assert torch.equal(out[rid], ref6[0])


# ---------------------------------------------------------------------------------------------------------------- end to end vs the oracle
def _restated_noises(keys, T, zs):
    """[T+1 tensors [B, *zs]]: the oracle's noise list from the float64 restatement, rounded to fp32"""
    per = [P.draws(seed, stream, T, zs) for seed, stream in keys]     # [B][T+1, *zs]
    return [torch.from_numpy(np.stack([p[k] for p in per])) for k in range(T + 1)]


@pytest.mark.parametrize("prec,min_latent_db", [("split", 90.0), ("fp32", 90.0), ("fp16", 40.0)])
def test_p_sample_loop_seeds_vs_oracle_fed_the_restatement(gpu, prec, min_latent_db):
    from resshift_amd import create_gaussian_diffusion

    up, ap, dp, _ = H.CASES["tiny"]
    um, am, usd, asd = _shells("tiny", gpu)
    y, _, _ = H.case_inputs(up, ap, dp, False, B=3)
    keys = _keys(3, base=2024)
    T = dp["steps"]
    ref, aux = oc.sample_loop(usd, up, asd, ap, dp, y, _restated_noises(keys, T, (3, 16, 16)), return_aux=True)
    d = create_gaussian_diffusion(**dp)
    d.set_precision(prec, prec, prec)
    out, g = d.p_sample_loop(y.to(gpu), um, first_stage_model=am, clip_denoised=False, model_kwargs={"lq": y.to(gpu)}, seeds=keys, return_aux=True)
    torch.cuda.synchronize()
    for b in range(3):
        zr, zg = aux["z_final"][b].double(), g["z_final"][b].cpu().double()
        mse = torch.mean((zg - zr) ** 2).item()
        latent_db = 10 * np.log10((zr.max() - zr.min()).item() ** 2 / max(mse, 1e-30))
        print(f"p_sample_loop(seeds=) {prec} image {b}: latent PSNR {latent_db:.1f} dB vs the oracle fed the restatement")
        assert latent_db >= min_latent_db, (b, latent_db)
    # the progressive path (clip_denoised) draws the same normals, one rs_noise_fill per draw: its first step's sample starts from the same x_T
    with pytest.raises(ValueError, match="excludes"):
        d.p_sample_loop(y.to(gpu), um, first_stage_model=am, clip_denoised=False, model_kwargs={"lq": y.to(gpu)}, seeds=keys, noise_repeat=True)
    d.set_precision("split", "split", "fp16")
    prog = d.p_sample_loop(y.to(gpu), um, first_stage_model=am, clip_denoised=True, model_kwargs={"lq": y.to(gpu)}, seeds=keys)
    torch.cuda.synchronize()
    assert tuple(prog.shape) == tuple(ref.shape) and torch.isfinite(prog).all()


def test_realsr_seeds_vs_oracle_at_the_parity_policy(gpu):
    """realsr B = 4, parity policy (split encoder + UNet, fp16 decoder), the project's criterion: every image >= 60 dB and >= 99.9 % of its
    VQ codes against oracle.sample_loop on the CPU fed the restatement's normals"""
    r = _realsr(gpu)
    up, ap, dp, d = r["up"], r["ap"], r["dp"], r["d"]
    T, B = d.num_timesteps, 4
    y, _, _ = H.synth.synthetic_inputs(H.SEED_X + 2, B, 64, 64, ap["embed_dim"], 64, 64, T)
    keys = _keys(B, base=77)
    ref, aux = oc.sample_loop(r["usd"], up, r["asd"], ap, dp, y, _restated_noises(keys, T, (3, 64, 64)), return_aux=True)
    d.set_precision(["split"] * T, "split", "fp16")
    out, g = d.p_sample_loop(y.to(gpu), r["um"], first_stage_model=r["am"], clip_denoised=False, model_kwargs={"lq": y.to(gpu)}, seeds=keys,
                             return_aux=True)
    torch.cuda.synchronize()
    idx, ridx = g["indices"].cpu().long().view(B, -1), aux["indices"].long().view(B, -1)
    for b in range(B):
        p = H.psnr(out[b:b + 1].cpu().clamp(-1, 1), ref[b:b + 1].clamp(-1, 1))
        agree = (idx[b] == ridx[b]).float().mean().item()
        print(f"realsr seeded, parity policy, image {b}: PSNR {p:.1f} dB, VQ agreement {agree:.5f}")
        assert p >= 60.0 and agree >= 0.999, (b, p, agree)

"""The oracle (oracle/resshift_oracle.py) against the committed golden outputs of the reference itself
(tests/golden/reference_outputs.npz, produced by oracle/make_golden.py from the reference tree; tests/golden/reference_checks.npz,
oracle/make_golden_checks.py, for the checks of its modules, configs, tiler and respaced schedule), plus — where the reference
modules can be imported — a live bit-exact re-check against the unmodified reference modules."""
import numpy as np
import pytest
import torch

import helpers as H
from oracle import ref_import, resshift_oracle as oc

torch.set_grad_enabled(False)


def test_schedule_known_answers():
    """SURVEY.md §8c known-answer vector + the reference's own tables stored in the golden file."""
    _, _, dp = H.realsr_params()
    s = oc.Schedule(dp)
    kat = [0.02, 0.11716508, 0.17630456, 0.23362892, 0.29157413, 0.35100928, 0.41235614, 0.47585773, 0.54167168, 0.60990993,
           0.68065802, 0.75398526, 0.82995066, 0.90860639, 0.99]
    assert np.allclose(s.sqrt_etas, kat, atol=1e-8)
    assert np.allclose(s.posterior_mean_coef1[1:4], [0.02913826, 0.44164095, 0.56947397], atol=1e-8)
    assert np.allclose(s.posterior_variance[1:3], [0.00155338, 0.03065984], atol=1e-8)
    assert s.timestep_map == list(range(15))
    g = H.golden()
    for k in ("sqrt_etas", "posterior_mean_coef1", "posterior_mean_coef2", "posterior_variance", "posterior_log_variance_clipped"):
        assert np.array_equal(getattr(s, k), g[f"sched/realsr_swinunet_realesrgan256/{k}"])


def test_product_schedule_matches_reference_tables():
    from resshift_amd.gaussian_diffusion import create_gaussian_diffusion

    g = H.golden()
    for cname in ("realsr_swinunet_realesrgan256", "realsr_swinunet_realesrgan256_journal"):
        dp = H.to_plain(H.load_config(cname))["diffusion"]["params"]
        d = create_gaussian_diffusion(**dp)
        for k in ("sqrt_etas", "posterior_mean_coef1", "posterior_mean_coef2", "posterior_variance", "posterior_log_variance_clipped"):
            assert np.array_equal(getattr(d, k), g[f"sched/{cname}/{k}"]), (cname, k)


@pytest.mark.parametrize("tag", list(H.CASES))
def test_oracle_tiny_cases_match_reference_outputs(tag):
    up, ap, dp, with_mask = H.CASES[tag]
    g = H.golden()
    usd, asd = H.weights(up, ap)
    y, noises, mask = H.case_inputs(up, ap, dp, with_mask)
    x, t = noises[1] * 1.3, torch.tensor([2, 2])
    kw = {"lq": y}
    if with_mask:
        kw["mask"] = mask
    assert H.rel_err(oc.unet_forward(usd, up, x, t, **kw), torch.from_numpy(g[f"{tag}/unet"])) < 2e-5
    img = torch.from_numpy(np.random.Generator(np.random.PCG64(7)).random((2, 3, 64, 64), dtype=np.float32) * 2 - 1)
    assert H.rel_err(oc.vq_encode(asd, ap, img), torch.from_numpy(g[f"{tag}/encode"])) < 2e-5
    d, idx = oc.vq_decode(asd, ap, noises[2] * 0.8, return_indices=True)
    assert H.rel_err(d, torch.from_numpy(g[f"{tag}/decode"])) < 2e-5
    assert np.array_equal(idx.numpy().astype(np.int32), g[f"{tag}/decode_idx"])
    out, aux = oc.sample_loop(usd, up, asd, ap, dp, y, noises, mask=mask, return_aux=True)
    assert H.rel_err(aux["z_final"], torch.from_numpy(g[f"{tag}/sample_z"])) < 5e-5
    assert (aux["indices"].numpy() == g[f"{tag}/sample_idx"]).mean() >= 0.995
    assert H.psnr(out.clamp(-1, 1), torch.from_numpy(g[f"{tag}/sample"]).clamp(-1, 1)) > 70.0


def test_oracle_full_size_realsr_matches_reference_output():
    """64x64 -> 256x256, 15 steps, B=1: the headline configuration at full size."""
    up, ap, dp = H.realsr_params()
    g = H.golden()
    usd, asd = H.weights(up, ap)
    y, noises, _ = H.synth.synthetic_inputs(H.SEED_X, 1, 64, 64, 3, 64, 64, dp["steps"])
    assert H.rel_err(oc.unet_forward(usd, up, noises[1] * 1.3, torch.tensor([7]), lq=y), torch.from_numpy(g["realsr/unet"])) < 2e-5
    out, aux = oc.sample_loop(usd, up, asd, ap, dp, y, noises, return_aux=True)
    assert H.rel_err(aux["z_final"], torch.from_numpy(g["realsr/sample_z"])) < 1e-4
    agree = (aux["indices"].numpy() == g["realsr/sample_idx"].astype(np.int64)).mean()
    assert agree >= 0.995, agree
    assert H.psnr(out.clamp(-1, 1), torch.from_numpy(g["realsr/sample"].astype(np.float32)).clamp(-1, 1)) > 60.0


@pytest.mark.parametrize("tag", ["tiny@48x32", "tiny@32x16", "tiny_fe@32x48"])
def test_oracle_offsize_matches_reference_outputs(tag):
    """The resolution-generic path: the networks run at a latent size other than the constructed one -
    per-size SW-MSA masks with the construction-time shift (models/swin_transformer.py:189-194,214-262), non-square maps.
    tests/golden/reference_offsize.npz holds the unmodified reference modules' outputs (oracle/make_golden_offsize.py)."""
    from oracle import make_golden_offsize as mo

    g = np.load(mo.os.path.join(mo.GOLD, "reference_offsize.npz"))
    up, ap, dp, with_mask, B, hz, wz = mo.TINY_CASES[tag]
    usd, asd = H.weights(up, ap)
    y, noises, mask = mo.case_inputs(tag)
    kw = {"lq": y}
    if with_mask:
        kw["mask"] = mask
    assert H.rel_err(oc.unet_forward(usd, up, noises[1] * 1.3, torch.tensor([2] * B), **kw), torch.from_numpy(g[f"{tag}/unet"])) < 2e-5
    out, aux = oc.sample_loop(usd, up, asd, ap, dp, y, noises, mask=mask, return_aux=True)
    assert H.rel_err(aux["z_final"], torch.from_numpy(g[f"{tag}/sample_z"])) < 5e-5
    assert (aux["indices"].numpy() == g[f"{tag}/sample_idx"]).mean() >= 0.995
    assert H.psnr(out.clamp(-1, 1), torch.from_numpy(g[f"{tag}/sample"]).clamp(-1, 1)) > 70.0


def test_oracle_offsize_full_network_and_tiles():
    """The headline network (constructed for 64 x 64 latents) on a 128 x 128 latent: one UNet forward against the reference's
    output (the 15-step loop at this size is pinned when the fixture is generated: 57 s of reference time); and the tiled path
    with 32-pixel tiles of the tiny network (tile latent 32 x 32, constructed 16 x 16) against the reference's ImageSpliterTh."""
    from oracle import make_golden_offsize as mo

    g = np.load(mo.os.path.join(mo.GOLD, "reference_offsize.npz"))
    up, ap, dp = H.realsr_params()
    usd, _ = H.weights(up, ap)
    y, noises, _ = mo.realsr_inputs(dp["steps"])
    assert H.rel_err(oc.unet_forward(usd, up, noises[1] * 1.3, torch.tensor([7]), lq=y), torch.from_numpy(g["realsr128/unet"])) < 2e-5
    up, ap, dp, _ = H.CASES["tiny"]
    usd, asd = H.weights(up, ap)
    y, calls = mo.tiled_inputs(dp["steps"])
    T = mo.TILED
    got = oc.sample_tiled(usd, up, asd, ap, dp, y, calls, chop_size=T["chop_size"], chop_stride=T["chop_stride"], chop_bs=T["chop_bs"],
                          padding_offset=T["padding_offset"])
    assert (got - torch.from_numpy(g["tiled32/sample"])).abs().max().item() <= 2e-5


@pytest.mark.parametrize("h,w", [(64, 128), (128, 64)])
def test_oracle_nonsquare_full_network(h, w):
    """The headline network on the smallest non-square planes its four levels and 8-pixel windows allow - the tile pool's size classes: one
    UNet forward (B = 1, t = 7) against the unmodified reference modules' output (tests/golden/reference_nonsquare.npz,
    oracle/make_golden_offsize.py).  The block-by-block GPU tests take the oracle as their reference at these shapes."""
    from oracle import make_golden_offsize as mo

    assert (h, w) in mo.NONSQUARE
    g = np.load(mo.os.path.join(mo.GOLD, "reference_nonsquare.npz"))
    up, ap, dp = H.realsr_params()
    usd, _ = H.weights(up, ap)
    x, y = mo.nonsquare_inputs(h, w, dp["steps"])
    ref = torch.from_numpy(g[f"realsr{h}x{w}/unet"])
    assert ref.shape == (1, 3, h, w) and ref.dtype == torch.float32
    assert H.rel_err(oc.unet_forward(usd, up, x, torch.tensor([7]), lq=y), ref) < 2e-5


def _checks():
    """tests/golden/reference_checks.npz: what the unmodified reference produced for the tests below (oracle/make_golden_checks.py, which
    also asserts the oracle bit-exact against every entry in the same run)"""
    from oracle import make_golden_checks as mc

    return np.load(mc.PATH)


def test_oracle_offsize_live_against_reference_modules():
    """the reference UNet at 48 x 32, 32 x 16 and 16 x 48 on a network constructed for 16 x 16: against its stored outputs, and bit-exact
    against the live modules where they can be imported (equal bits need the host the stored outputs were made on: thread count and ISA
    change the reduction order)"""
    from oracle import make_golden_checks as mc

    g = _checks()
    up = mc.cases.TINY_UNET
    usd, _ = mc.tiny_weights()
    um = None
    if ref_import.available():
        U, _, _ = ref_import.load()
        um = U(**up).eval()
        um.load_state_dict(usd, strict=True)
    for (h, w, x, y) in mc.offsize_inputs():
        got = oc.unet_forward(usd, up, x, torch.tensor([1, 1]), lq=y)
        assert H.rel_err(got, torch.from_numpy(g[f"offsize/{h}x{w}"])) < 2e-5, (h, w)
        if um is not None:
            assert torch.equal(got, um(x, torch.tensor([1, 1]), lq=y)), (h, w)


def test_oracle_live_against_reference_modules():
    """the tiny UNet forward and VQ-f4 encoder against the reference's stored outputs (and the UNet bit-exact against the live modules
    where they can be imported)"""
    from oracle import make_golden_checks as mc

    g = _checks()
    up, ap = mc.cases.TINY_UNET, mc.cases.TINY_AE
    usd, asd = mc.tiny_weights()
    x, t, y, img = mc.live_inputs()
    got = oc.unet_forward(usd, up, x, t, lq=y)
    assert H.rel_err(got, torch.from_numpy(g["live/unet"])) < 2e-5
    assert H.rel_err(oc.vq_encode(asd, ap, img), torch.from_numpy(g["live/encode"])) < 2e-5
    if ref_import.available():
        U, _, _ = ref_import.load()
        um = U(**up).eval()
        um.load_state_dict(usd, strict=True)
        assert torch.equal(got, um(x, t, lq=y))


@pytest.mark.parametrize("cname", ["realsr_swinunet_realesrgan256", "faceir_gfpgan512_lpips", "inpaint_lama256_imagenet"])
def test_spec_equals_reference_state_dict(cname):
    """resshift_amd.spec must list exactly the reference's state_dict keys, shapes and order (stored from the reference's own modules built
    from its own configs/<cname>.yaml), and the config digest must equal that YAML."""
    import json

    ref = json.loads(str(_checks()[f"spec/{cname}"]))
    mine = H.to_plain(H.load_config(cname))
    for sec in ("model", "diffusion", "autoencoder"):
        assert ref["config"][sec] == mine[sec], f"config digest drifted from the reference YAML: {cname}/{sec}"
    spec, _ = H.unet_param_spec(mine["model"]["params"])
    assert [(k, tuple(s)) for k, s in ref["unet"]] == list(spec.items())
    assert [(k, tuple(s)) for k, s in ref["ae"]] == list(H.ae_param_spec(mine["autoencoder"]["params"]).items())


def test_tiling_restatements_against_reference_ImageSpliterTh():
    """utils/util_image.py ImageSpliterTh, as stored by oracle/make_golden_checks.py: the oracle's and the product's tile origin lists must be
    its lists, the patches cut at its canvas windows must be the patches it handed out, and the sum/count averaging of the deterministic
    per-tile results must reproduce its gather() bit for bit."""
    import hashlib
    import json

    from oracle import make_golden_checks as mc
    from resshift_amd.tiling import extract_starts

    g = _checks()
    for k, (Hh, W, ps, st, sf, ebs) in enumerate(mc.TILING_CASES):
        assert list(g[f"tiling/{k}/height_starts"]) == oc.tile_starts(Hh, ps, st) == extract_starts(Hh, ps, st)
        assert list(g[f"tiling/{k}/width_starts"]) == oc.tile_starts(W, ps, st) == extract_starts(W, ps, st)
        windows = json.loads(str(g[f"tiling/{k}/windows"]))
        assert sum(len(c) for c in windows) == len(oc.tile_starts(Hh, ps, st)) * len(oc.tile_starts(W, ps, st))
        assert all(len(c) == ebs for c in windows[:-1]) and 0 < len(windows[-1]) <= ebs
        im = mc.tiling_image(k)
        res = torch.zeros(2, 3, Hh * sf, W * sf)
        cnt = torch.zeros_like(res)
        pch_hash = hashlib.sha256()
        for infos in windows:
            pch = torch.cat([im[:, :, h0 // sf:h1 // sf, w0 // sf:w1 // sf] for (h0, h1, w0, w1) in infos])
            pch_hash.update(pch.contiguous().numpy().tobytes())
            out = mc.tiling_result(pch, sf)
            for t, (h0, h1, w0, w1) in enumerate(infos):
                res[:, :, h0:h1, w0:w1] += out[t * 2:(t + 1) * 2]
                cnt[:, :, h0:h1, w0:w1] += 1
        assert pch_hash.hexdigest() == str(g[f"tiling/{k}/pch_sha256"]), k
        assert bool((cnt > 0).all()) and mc.digest(res / cnt) == str(g[f"tiling/{k}/gather_sha256"]), k


def test_tiled_path_oracle_vs_reference_golden():
    """tests/golden/reference_tiled.npz was produced by the reference's own ImageSpliterTh + UNet / VQ-AE / diffusion loop
    (oracle/make_golden_tiled.py); the oracle's tiled restatement must reproduce it wherever the tests run."""
    import os

    from oracle import make_golden_tiled as mt

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_tiled.npz"))
    assert list(g["meta"]) == [mt.CHOP_SIZE, mt.CHOP_STRIDE, mt.CHOP_BS, mt.PAD_OFFSET, mt.SEED]
    up, ap, dp, _ = H.CASES["tiny"]
    usd, asd = H.weights(up, ap)
    y, calls = mt.tiled_inputs(dp["steps"])
    got = oc.sample_tiled(usd, up, asd, ap, dp, y, calls, chop_size=mt.CHOP_SIZE, chop_stride=mt.CHOP_STRIDE, chop_bs=mt.CHOP_BS,
                          padding_offset=mt.PAD_OFFSET)
    assert (got - torch.from_numpy(g["sample"])).abs().max().item() <= 2e-5


def test_respaced_schedule_live_against_reference():
    """timestep_respacing < steps (respace.py:23-70): the oracle's and the product's tables and timestep map against the ones the
    reference's own SpacedDiffusion object holds (stored by oracle/make_golden_checks.py)."""
    from oracle import make_golden_checks as mc
    from resshift_amd import create_gaussian_diffusion

    g = _checks()
    dp = dict(mc.RESPACE_DP)
    s = oc.Schedule(dp)
    mine = create_gaussian_diffusion(**dp)
    assert list(g["respace/timestep_map"]) == s.timestep_map == mine.timestep_map == [0, 3, 6, 9]
    for name in mc.RESPACE_TABLES:
        r = g[f"respace/{name}"]
        assert np.array_equal(r, np.asarray(getattr(s, name), dtype=np.float64)), name
        assert np.array_equal(r, np.asarray(getattr(mine, name), dtype=np.float64)), name


@pytest.mark.skipif(not ref_import.available(), reason="reference modules (tree or verified oracle/_ref copy) not present")
def test_reference_baseline_wrapper_runs_the_reference_loop_and_agrees_with_the_oracle(capsys):
    """bench.py's baseline legs (oracle/ref_baseline.py: `cpu_baseline.kind = "reference"`, `torch_rocm_autocast_baseline`) drive the UNMODIFIED
    modules' p_sample_loop_progressive + decode_first_stage with injected noise.  On the tiny case: same image / latent / VQ indices as the
    oracle's restatement (which is pinned to the reference elsewhere in this file), and nothing on stdout - bench.py's stdout is ONE JSON line
    and the reference prints notices while it is imported and constructed."""
    from oracle import ref_baseline

    up, ap, dp, _ = H.CASES["tiny"]
    usd, asd = H.weights(up, ap)
    y, noises, _ = H.synth.synthetic_inputs(H.SEED_X, 2, 16, 16, ap["embed_dim"], 16, 16, dp["steps"])
    capsys.readouterr()
    ref = ref_baseline.Reference(up, ap, dp, usd, asd)
    img, z, idx = ref.sample(y, noises)
    assert capsys.readouterr().out == ""
    o_img, aux = oc.sample_loop(usd, up, asd, ap, dp, y, noises, return_aux=True)
    assert torch.equal(idx, aux["indices"].reshape(2, -1))
    assert (img - o_img).abs().max().item() < 1e-4 and (z - aux["z_final"]).abs().max().item() < 1e-4


def test_winograd_study_transform_is_the_direct_convolution():
    """oracle/study_winograd.py decides a kernel design on the CPU; its F(2x2, 3x3) emulation must BE a 3x3 / pad-1 convolution:
    fp32 operands reproduce F.conv2d to fp32 rounding, pair operands to the pair's 2^-22."""
    from oracle import study_winograd as sw

    g = torch.Generator().manual_seed(3)
    x, w, b = torch.randn(2, 32, 8, 12, generator=g), torch.randn(48, 32, 3, 3, generator=g) / 17.0, torch.randn(48, generator=g)
    ref = torch.nn.functional.conv2d(x.double(), w.double(), b.double(), padding=1)
    sd = {"t.weight": w, "t.bias": b}
    for split, tol in ((False, 2e-6), (True, 4e-6)):
        sw._U.clear()
        got = sw.wino(sd, "t", x, split)
        assert (got.double() - ref).abs().max().item() / ref.abs().max().item() < tol

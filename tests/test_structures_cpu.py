"""The network structures of oracle/cases.py: STRUCTURES - graphs off the two the rest of the suite builds - without a GPU: the oracle and the
parameter spec against what the unmodified reference modules gave (tests/golden/reference_structures.npz, oracle/make_golden_structures.py),
the engine's whole control flow on the fake device for every case tests/test_structures_gpu.py runs (tests/_fake_device_structures.py),
and the configurations the engine refuses."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _structures as T
import helpers as H
from oracle import cases, resshift_oracle as oc

torch.set_grad_enabled(False)
S = T.S
NO_GPU = {"HIP_VISIBLE_DEVICES": "-1"}   # (the child processes see no HIP device, also when the suite runs on a GPU machine)


@pytest.mark.parametrize("tag", list(S["unet"]))
def test_oracle_and_spec_reproduce_the_reference_unet(tag):
    """one forward at B = 2 with two different timesteps, and the state_dict's names, shapes and order"""
    from oracle import make_golden_structures as ms

    g, up = T.fixture(), S["unet"][tag]
    x, t, kw = ms.unet_inputs(tag)
    assert len(set(t.tolist())) == 2
    ref = torch.from_numpy(g[f"unet/{tag}"])
    assert ref.dtype == torch.float32 and ref.shape == (2, up["out_channels"], up["image_size"], up["image_size"])
    assert H.rel_err(oc.unet_forward(T.unet_weights(up), up, x, t, **kw), ref) < 2e-5
    spec, buffers = H.unet_param_spec(up)
    assert [(k, tuple(s)) for k, s in json.loads(str(g[f"keys/unet/{tag}"]))] == list(spec.items())


@pytest.mark.parametrize("tag", list(S["ae"]))
def test_oracle_and_spec_reproduce_the_reference_autoencoder(tag):
    from oracle import make_golden_structures as ms

    g, ap = T.fixture(), S["ae"][tag]
    asd = T.ae_weights(ap)
    img, z = ms.ae_inputs(tag)
    assert H.rel_err(oc.vq_encode(asd, ap, img), torch.from_numpy(g[f"ae/{tag}/encode"])) < 2e-5
    d, idx = oc.vq_decode(asd, ap, z, return_indices=True)
    assert H.rel_err(d, torch.from_numpy(g[f"ae/{tag}/decode"])) < 2e-5
    assert np.array_equal(idx.numpy().astype(np.int32), g[f"ae/{tag}/decode_idx"])
    assert [(k, tuple(s)) for k, s in json.loads(str(g[f"keys/ae/{tag}"]))] == list(H.ae_param_spec(ap).items())


@pytest.mark.parametrize("tag", list(S["pairs"]))
def test_oracle_reproduces_the_reference_loop(tag):
    from oracle import make_golden_structures as ms

    g = T.fixture()
    up, ap, dp, with_mask = cases.structure_pair(tag)
    y, noises, mask = ms.pair_inputs(tag)
    assert (mask is not None) == with_mask
    out, aux = oc.sample_loop(T.unet_weights(up), up, T.ae_weights(ap), ap, dp, y, noises, mask=mask, return_aux=True)
    assert H.rel_err(aux["z_final"], torch.from_numpy(g[f"pair/{tag}/sample_z"])) < 5e-5
    assert (aux["indices"].numpy() == g[f"pair/{tag}/sample_idx"]).mean() >= 0.995
    assert H.psnr(out.clamp(-1, 1), torch.from_numpy(g[f"pair/{tag}/sample"].astype(np.float32)).clamp(-1, 1)) > 70.0


def test_fixture_is_small_and_fp32():
    """under 512 KiB; fp32 wherever the comparison is at 1e-5 (the 128 x 128 loop image alone is fp16: it is compared in dB)"""
    from oracle import make_golden_structures as ms

    assert os.path.getsize(ms.PATH) < 512 * 1024
    g = T.fixture()
    for k in g.files:
        if k.startswith(("unet/", "ae/")) and not k.endswith("_idx") or k.endswith("/sample_z"):
            assert g[k].dtype == np.float32, k


# The launch mix of every case on the fake device: "<call>:<structure>:<batch>:<precision code>[:<h>x<w>]" -> (kernel launches, launches
# per kernel family in the order of Exec::Fam / Engine.FAMILIES, igemm-path launches, GroupNorm launches), as the routing rules gave them
# when these structures were added.  A change of kernel choice on these graphs has to show up here, on purpose.  What it says today: none of
# the small planes takes the halo or Winograd kernels; the heads6_* structures run the fused attention (families 5 / 7) in fp16 and split
# storage at every batch and the fused MLP (6 / 8) on the 32 x 32 level's four blocks at B = 16 only - 46 implicit GEMMs there against 54 at
# B = 2, and the same 46 with model_channels 128 and 192: patch_unembed stays a 1x1 conv launch of its own (the fold is for 160 channels).
MIX = {
    "unet:one_level:3:2": (66, [0, 0, 0, 36, 0, 0, 0, 0, 0, 0, 0, 0], 36, 20),
    "unet:one_level:3:0": (66, [0, 0, 36, 0, 0, 0, 0, 0, 0, 0, 0, 0], 36, 21),
    "unet:one_level:3:1": (69, [0, 0, 0, 0, 36, 0, 0, 0, 0, 0, 0, 0], 36, 21),
    "unet:one_level:2:0": (66, [0, 0, 36, 0, 0, 0, 0, 0, 0, 0, 0, 0], 36, 21),
    "unet:one_level:2:1": (69, [0, 0, 0, 0, 36, 0, 0, 0, 0, 0, 0, 0], 36, 21),
    "unet:one_level:2:2": (66, [0, 0, 0, 36, 0, 0, 0, 0, 0, 0, 0, 0], 36, 20),
    "unet:three_uneven:3:2": (141, [0, 0, 0, 79, 0, 0, 0, 0, 0, 0, 0, 0], 79, 46),
    "unet:three_uneven:3:0": (142, [0, 0, 79, 0, 0, 0, 0, 0, 0, 0, 0, 0], 79, 47),
    "unet:three_uneven:3:1": (162, [0, 0, 0, 0, 79, 0, 0, 0, 0, 0, 0, 0], 79, 47),
    "unet:three_uneven:2:2:64x32": (141, [0, 0, 0, 79, 0, 0, 0, 0, 0, 0, 0, 0], 79, 46),
    "unet:three_uneven:2:0": (142, [0, 0, 79, 0, 0, 0, 0, 0, 0, 0, 0, 0], 79, 47),
    "unet:three_uneven:2:1": (162, [0, 0, 0, 0, 79, 0, 0, 0, 0, 0, 0, 0], 79, 47),
    "unet:three_uneven:2:2": (141, [0, 0, 0, 79, 0, 0, 0, 0, 0, 0, 0, 0], 79, 46),
    "unet:mult0:3:2": (109, [0, 0, 0, 59, 0, 0, 0, 0, 0, 0, 0, 0], 59, 32),
    "unet:mult0:3:0": (109, [0, 0, 59, 0, 0, 0, 0, 0, 0, 0, 0, 0], 59, 33),
    "unet:mult0:3:1": (126, [0, 0, 0, 0, 59, 0, 0, 0, 0, 0, 0, 0], 59, 33),
    "unet:mult0:2:0": (109, [0, 0, 59, 0, 0, 0, 0, 0, 0, 0, 0, 0], 59, 33),
    "unet:mult0:2:1": (126, [0, 0, 0, 0, 59, 0, 0, 0, 0, 0, 0, 0], 59, 33),
    "unet:mult0:2:2": (109, [0, 0, 0, 59, 0, 0, 0, 0, 0, 0, 0, 0], 59, 32),
    "unet:depth3:3:2": (163, [0, 0, 0, 94, 0, 0, 0, 0, 0, 0, 0, 0], 94, 46),
    "unet:depth3:3:0": (164, [0, 0, 94, 0, 0, 0, 0, 0, 0, 0, 0, 0], 94, 47),
    "unet:depth3:3:1": (175, [0, 0, 0, 0, 94, 0, 0, 0, 0, 0, 0, 0], 94, 47),
    "unet:depth3:2:0": (164, [0, 0, 94, 0, 0, 0, 0, 0, 0, 0, 0, 0], 94, 47),
    "unet:depth3:2:1": (175, [0, 0, 0, 0, 94, 0, 0, 0, 0, 0, 0, 0], 94, 47),
    "unet:depth3:2:2": (163, [0, 0, 0, 94, 0, 0, 0, 0, 0, 0, 0, 0], 94, 46),
    "unet:no_level_attn:3:2": (64, [0, 0, 0, 34, 0, 0, 0, 0, 0, 0, 0, 0], 34, 20),
    "unet:no_level_attn:3:0": (64, [0, 0, 34, 0, 0, 0, 0, 0, 0, 0, 0, 0], 34, 21),
    "unet:no_level_attn:3:1": (75, [0, 0, 0, 0, 34, 0, 0, 0, 0, 0, 0, 0], 34, 21),
    "unet:no_level_attn:2:0": (64, [0, 0, 34, 0, 0, 0, 0, 0, 0, 0, 0, 0], 34, 21),
    "unet:no_level_attn:2:1": (75, [0, 0, 0, 0, 34, 0, 0, 0, 0, 0, 0, 0], 34, 21),
    "unet:no_level_attn:2:2": (64, [0, 0, 0, 34, 0, 0, 0, 0, 0, 0, 0, 0], 34, 20),
    "unet:fe1_mask:3:2": (131, [0, 0, 0, 75, 0, 0, 0, 0, 0, 0, 0, 0], 75, 36),
    "unet:fe1_mask:3:0": (131, [0, 0, 75, 0, 0, 0, 0, 0, 0, 0, 0, 0], 75, 37),
    "unet:fe1_mask:3:1": (142, [0, 0, 0, 0, 75, 0, 0, 0, 0, 0, 0, 0], 75, 37),
    "unet:fe1_mask:2:0": (131, [0, 0, 75, 0, 0, 0, 0, 0, 0, 0, 0, 0], 75, 37),
    "unet:fe1_mask:2:1": (142, [0, 0, 0, 0, 75, 0, 0, 0, 0, 0, 0, 0], 75, 37),
    "unet:fe1_mask:2:2": (131, [0, 0, 0, 75, 0, 0, 0, 0, 0, 0, 0, 0], 75, 36),
    "unet:heads6_mc128:16:2": (109, [0, 0, 0, 46, 0, 0, 0, 10, 4, 0, 0, 0], 60, 25),
    "unet:heads6_mc128:16:0": (121, [0, 0, 46, 0, 0, 10, 4, 0, 0, 0, 0, 0], 60, 37),
    "unet:heads6_mc128:16:1": (156, [0, 0, 0, 0, 74, 0, 0, 0, 0, 0, 0, 0], 74, 37),
    "unet:heads6_mc128:2:2": (120, [0, 0, 0, 54, 0, 0, 0, 10, 0, 0, 0, 0], 64, 31),
    "unet:heads6_mc128:2:0": (126, [0, 0, 54, 0, 0, 10, 0, 0, 0, 0, 0, 0], 64, 37),
    "unet:heads6_mc128:2:1": (157, [0, 0, 0, 0, 74, 0, 0, 0, 0, 0, 0, 0], 74, 37),
    "unet:heads6_mc192:16:2": (109, [0, 0, 0, 46, 0, 0, 0, 10, 4, 0, 0, 0], 60, 25),
    "unet:heads6_mc192:16:0": (121, [0, 0, 46, 0, 0, 10, 4, 0, 0, 0, 0, 0], 60, 37),
    "unet:heads6_mc192:16:1": (158, [0, 0, 0, 0, 74, 0, 0, 0, 0, 0, 0, 0], 74, 37),
    "unet:heads6_mc192:2:2": (120, [0, 0, 0, 54, 0, 0, 0, 10, 0, 0, 0, 0], 64, 31),
    "unet:heads6_mc192:2:0": (126, [0, 0, 54, 0, 0, 10, 0, 0, 0, 0, 0, 0], 64, 37),
    "unet:heads6_mc192:2:1": (159, [0, 0, 0, 0, 74, 0, 0, 0, 0, 0, 0, 0], 74, 37),
    "encode:ae_f1:2:2:16x16": (27, [0, 0, 0, 13, 0, 0, 0, 0, 0, 0, 0, 0], 13, 7),
    "encode:ae_f1:2:0:16x16": (27, [0, 0, 13, 0, 0, 0, 0, 0, 0, 0, 0, 0], 13, 8),
    "encode:ae_f1:2:1:16x16": (27, [0, 0, 0, 0, 13, 0, 0, 0, 0, 0, 0, 0], 13, 8),
    "decode:ae_f1:2:2:16x16": (32, [0, 0, 0, 15, 0, 0, 0, 0, 0, 0, 0, 0], 15, 9),
    "decode:ae_f1:2:0:16x16": (32, [0, 0, 15, 0, 0, 0, 0, 0, 0, 0, 0, 0], 15, 10),
    "decode:ae_f1:2:1:16x16": (32, [0, 0, 0, 0, 15, 0, 0, 0, 0, 0, 0, 0], 15, 10),
    "encode:ae_f8_equal:2:2:128x128": (51, [0, 0, 0, 28, 0, 0, 0, 0, 0, 0, 0, 0], 28, 18),
    "encode:ae_f8_equal:2:0:128x128": (51, [0, 0, 28, 0, 0, 0, 0, 0, 0, 0, 0, 0], 28, 18),
    "encode:ae_f8_equal:2:1:128x128": (62, [0, 0, 0, 0, 28, 0, 0, 0, 0, 0, 0, 0], 28, 18),
    "decode:ae_f8_equal:2:2:16x16": (68, [0, 0, 0, 35, 0, 0, 0, 0, 0, 0, 0, 0], 35, 25),
    "decode:ae_f8_equal:2:0:16x16": (69, [0, 0, 35, 0, 0, 0, 0, 0, 0, 0, 0, 0], 35, 26),
    "decode:ae_f8_equal:2:1:16x16": (86, [0, 0, 0, 0, 35, 0, 0, 0, 0, 0, 0, 0], 35, 26),
    "encode:ae_f2_wide:2:2:32x32": (38, [0, 0, 0, 17, 0, 0, 0, 0, 0, 0, 0, 0], 17, 9),
    "encode:ae_f2_wide:2:0:32x32": (38, [0, 0, 17, 0, 0, 0, 0, 0, 0, 0, 0, 0], 17, 10),
    "encode:ae_f2_wide:2:1:32x32": (42, [0, 0, 0, 0, 17, 0, 0, 0, 0, 0, 0, 0], 17, 10),
    "decode:ae_f2_wide:2:2:16x16": (52, [0, 0, 0, 21, 0, 0, 0, 0, 0, 0, 0, 0], 21, 13),
    "decode:ae_f2_wide:2:0:16x16": (53, [0, 0, 21, 0, 0, 0, 0, 0, 0, 0, 0, 0], 21, 14),
    "decode:ae_f2_wide:2:1:16x16": (56, [0, 0, 0, 0, 21, 0, 0, 0, 0, 0, 0, 0], 21, 14),
    "sample:one_level+ae_f1:2:2": (319, [0, 0, 0, 172, 0, 0, 0, 0, 0, 0, 0, 0], 172, 96),
    "sample:one_level+ae_f1:2:0": (324, [0, 0, 172, 0, 0, 0, 0, 0, 0, 0, 0, 0], 172, 102),
    "sample:one_level+ae_f1:2:1": (336, [0, 0, 0, 0, 172, 0, 0, 0, 0, 0, 0, 0], 172, 102),
    "sample:fe1_mask+ae_f8_equal:2:2": (625, [0, 0, 0, 357, 0, 0, 0, 0, 0, 0, 0, 0], 357, 187),
    "sample:fe1_mask+ae_f8_equal:2:0": (630, [0, 0, 357, 0, 0, 0, 0, 0, 0, 0, 0, 0], 357, 192),
    "sample:fe1_mask+ae_f8_equal:2:1": (702, [0, 0, 0, 0, 357, 0, 0, 0, 0, 0, 0, 0], 357, 192),
}


def _all_args():
    return [(fam, tag) for fam in ("unet", "ae", "pairs") for tag in S[fam]]


def test_every_case_has_a_pinned_launch_mix():
    assert sorted(a for fam, tag in _all_args() for a in T.fake_args(fam, tag)) == sorted(MIX)


@pytest.mark.parametrize("family,tag", _all_args(), ids=[t for _, t in _all_args()])
def test_dry_and_real_pass_agree_on_every_structure_without_a_gpu(family, tag):
    """rs_unet_forward / rs_vq_encode / rs_vq_decode / rs_sample on the fake device, in fp16, fp32 and split storage, at B = 2 and at the batch
    (and plane) of the GPU test: the dry sizing pass and the real pass report equal tickets, pool bytes and producer / GroupNorm counts, no
    planned tail stays unattached, the call ends with the fake device's own failure (the first launch that fails: rc -1, "launch failed"),
    not with an internal error, and the launch mix is the pinned one."""
    from resshift_amd import build as _b

    args = T.fake_args(family, tag)
    env = dict(os.environ, RS_FAKE_DEVICE="1", RESSHIFT_HIP_LIB=_b.build_testhooks(), **NO_GPU)
    r = subprocess.run([sys.executable, os.path.join(H.ROOT, "tests", "_fake_device_structures.py")] + args, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    assert "never attached" not in r.stderr and "disagree" not in r.stdout + r.stderr, (r.stdout[-500:], r.stderr[-1500:])
    walked = dict(re.findall(r"^case (\S+)\n\[fake device\] (dry: .*)$", r.stderr, re.M))
    lines = {ln.split()[0]: ln for ln in r.stdout.splitlines()}
    assert list(lines) == args
    for a in args:
        m = re.search(r"dry: tickets (\d+) pool (\d+) prod (\d+) gn (\d+) \| real: tickets (\d+) pool (\d+) prod (\d+) gn (\d+) launches (\d+)", walked.get(a, ""))
        assert m, (a, r.stderr[-1500:])
        v = [int(x) for x in m.groups()]
        assert v[:4] == v[4:8], (a, v)
        f = re.match(r"\S+ rc (-?\d+) err (.*) launches (\d+) families ([\d,]+) igemm (\d+) gn (\d+)$", lines[a])
        assert f, lines[a]
        assert int(f.group(1)) == -1 and "launch failed" in f.group(2) and "internal" not in f.group(2), lines[a]
        got = (int(f.group(3)), [int(x) for x in f.group(4).split(",")], int(f.group(5)), int(f.group(6)))
        assert got == MIX[a], (a, got, MIX[a])


def _config(up=None, ap=None):
    from resshift_amd import _lib
    from resshift_amd.engine import _fill_ae, _fill_unet

    cfg = _lib.Config()
    if up is not None:
        _fill_unet(cfg.unet, up)
        cfg.has_unet = 1
    if ap is not None:
        _fill_ae(cfg.ae, ap)
        cfg.has_ae = 1
    cfg.enable_f16 = cfg.enable_f32 = cfg.enable_split = 1
    return cfg


REFUSED = [
    ("window_size", dict(cases.TINY_UNET, window_size=4), None),
    ("num_head_channels", dict(cases.TINY_UNET, num_head_channels=16), None),                           # 64 / 16: 4 heads of 16 channels
    ("channel_mult", dict(cases.TINY_UNET, channel_mult=[1, 2, 2], num_res_blocks=[1, 1, 1]), None),   # 16 -> 8 -> 4
    ("attn_resolutions", None, dict(cases.TINY_AE, ddconfig=dict(cases.TINY_AE["ddconfig"], attn_resolutions=[16]))),
    ("embed_dim", None, dict(cases.TINY_AE, embed_dim=6)),
    ("embed_dim", None, dict(cases.TINY_AE, embed_dim=16)),
    ("n_embed", None, dict(cases.TINY_AE, embed_dim=8, n_embed=8192)),                         # 8192 * 9 * 4 = 288 KiB
    ("n_embed", None, dict(cases.TINY_AE, embed_dim=3, n_embed=10241)),                        # one row over 160 KiB
]


@pytest.mark.parametrize("field,up,ap", REFUSED, ids=[f"{k}-{r[0].replace(' ', '_')}" for k, r in enumerate(REFUSED)])
def test_unsupported_configurations_are_refused_at_create(field, up, ap):
    """what the engine cannot run fails at rs_create - before any device is touched: this runs in a process that never sees one - with a
    message that names the field, not at the first call that reaches the missing kernel"""
    from resshift_amd import _lib

    lib = _lib.load()
    assert not lib.rs_create(ctypes.byref(_config(up, ap)))
    assert field in _lib.last_error(), _lib.last_error()


def test_supported_edges_are_accepted_at_create():
    """the neighbours of the refusals: every STRUCTURES entry, and the largest codebook that fits (10240 rows of 3 + 1 floats: 160 KiB)"""
    from resshift_amd import _lib

    lib = _lib.load()
    ok = [(up, None) for up in S["unet"].values()] + [(None, ap) for ap in S["ae"].values()] + [(None, dict(cases.TINY_AE, n_embed=10240))]
    for up, ap in ok:
        h = lib.rs_create(ctypes.byref(_config(up, ap)))
        assert h, _lib.last_error()
        lib.rs_destroy(h)

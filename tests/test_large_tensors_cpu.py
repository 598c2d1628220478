"""The host side of tests/test_large_tensors_gpu.py: what can be checked about tensors past 2^31 bytes without a device.

  * every operand of every GPU case is periodic with a period that neither 2^31 nor 2^32 bytes is a multiple of, and lies where its row of
    the case table says (between 2^31 bytes and RS_BUFFER_BYTES_LIMIT for the buffer-offset kernels, past 2^31 elements for GroupNorm and
    the layout kernels);
  * the wide rows (ld0 / ldy / ldres) by which the ops.conv2d cases reach those sizes leave the conv plan as it is, and the plan is the
    row's kernel;
  * a sweep of ops.conv_plan over the conv layers of every shipped config (derived from the YAML, autoencoder and UNet) at every batch 1 .. 256,
    and over the layer grid of tests/_conv_classes.py at the batches (up to 256) that put x0 between 2^31 bytes and the limit: which kernels a DENSE layer of that size plans onto, pinned - the others (igemm3, the halo kernel's small-plane geometry, every
    split-K class) are reached through wide rows only, and each has such a GPU case.  A planner change that moves either set fails here;
  * the engine refuses an oversize operand while it PLANS: on the fake device (tests/_fake_device_limit.py) the shipped autoencoders at the
    first batch at which their largest conv operand reaches the limit - computed from the config: faceir's encoder in split storage at
    60, realsr's at 120, realsr's fp16 decoder at 120 too (its last level's first conv reads 256 channels at full resolution) - fail in the dry pass with the named text and zero
    launches, and the batch below walks through to the fake device's own failure."""
import os
import re
import subprocess
import sys

import pytest

import _conv_classes as CC
import _large as LG
import helpers as H

pytestmark = pytest.mark.skipif(bool(CC.planner_env()), reason=f"planner knobs set in the environment: {CC.planner_env()}")
NO_GPU = {"HIP_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": "", "CUDA_VISIBLE_DEVICES": ""}
BUFFER_KERNELS = ("CK_IGEMM2", "CK_IGEMM3", "CK_HALO", "CK_HALO_SEG", "CK_SPLIT", "CK_WINO")


@pytest.fixture(scope="module", autouse=True)
def _built():
    from resshift_amd import build

    build.build(verbose=False)


def test_limit_constant_matches_the_library_source():
    src = open(os.path.join(H.ROOT, "resshift_amd", "csrc", "common.h")).read()
    assert re.search(r"#define RS_BUFFER_BYTES_LIMIT 0x([0-9A-Fa-f]+)ull", src) and int(re.search(r"#define RS_BUFFER_BYTES_LIMIT 0x([0-9A-Fa-f]+)ull", src).group(1), 16) == LG.LIMIT
    # ... and no kernel file spells the value out again
    for name in os.listdir(os.path.join(H.ROOT, "resshift_amd", "csrc")):
        if name != "common.h" and name.endswith((".h", ".hip")):
            assert "0xf0000000" not in open(os.path.join(H.ROOT, "resshift_amd", "csrc", name)).read().lower(), name


@pytest.mark.parametrize("c", LG.CONV_CASES + LG.BOUNDARY_CONV, ids=[c.name for c in LG.CONV_CASES] + ["boundary-" + c.name for c in LG.BOUNDARY_CONV])
def test_conv_case_sizes_aliasing_and_plan(c):
    per = LG.conv_bytes(c)
    for o in ("x", "y", "res"):
        if per[o]:
            assert LG.alias_visible(per[o]), (c.name, o, per[o])
    for o in c.big.split():
        n = c.L.B * per[o]
        assert n > LG.G31, (c.name, o, n)
        if c.kernel in BUFFER_KERNELS:
            assert n < LG.LIMIT, (c.name, o, n)
    plan = LG.conv_plan_of(c)
    assert plan is not None and plan.kernel == c.kernel and (plan.splitk > 1) == c.sk, (c.name, plan)
    assert plan == LG.conv_plan_of(c, dense=True), "the wide rows changed the plan"
    # the refused neighbour of a boundary case plans the same launch: it is the launcher, not the planner, that knows the limit
    if c in LG.BOUNDARY_CONV:
        assert LG.conv_plan_of(c._replace(L=c.L._replace(B=c.L.B + 1))).kernel == c.kernel
        assert c.L.B * per["x"] < LG.LIMIT <= (c.L.B + 1) * per["x"]


def test_dense_case_sizes_and_aliasing():
    E = 192
    rows = [("halo-f16", LG.HALO_F16, LG.HALO_F16[3], 2, True), ("halo-split", LG.HALO_SPLIT, LG.HALO_SPLIT[3], 4, True),
            ("wino-split", LG.WINO_SPLIT, LG.WINO_SPLIT[3], 4, True), ("wino-boundary", LG.WINO_BOUNDARY, LG.WINO_BOUNDARY[3], 4, True),
            ("attn-f16", LG.ATTN_F16, E, 2, True), ("attn-split", LG.ATTN_SPLIT, E, 4, True),
            ("attn-f16-boundary", LG.ATTN_F16_BOUNDARY, E, 2, True), ("attn-split-boundary", LG.ATTN_SPLIT_BOUNDARY, E, 4, True),
            ("mlp-f16", (LG.MLP_F16[0], LG.MLP_F16[1], 1), E, 2, False), ("mlp-split", (LG.MLP_SPLIT[0], LG.MLP_SPLIT[1], 1), E, 4, False),
            ("groupnorm-f16", LG.GN_SHAPE, LG.GN_SHAPE[3], 2, False), ("groupnorm-split", LG.GN_SHAPE, LG.GN_SHAPE[3], 4, False),
            ("layout-f16", LG.ELEMENTWISE_SHAPE, LG.ELEMENTWISE_SHAPE[3], 2, False), ("layout-f32", LG.ELEMENTWISE_SHAPE, LG.ELEMENTWISE_SHAPE[3], 4, False)]
    for name, shape, C, esz, limited in rows:
        per = LG.dense_bytes(shape, C, esz)
        assert LG.alias_visible(per), (name, per)
        assert shape[0] * per > LG.G31 and (not limited or shape[0] * per < LG.LIMIT), (name, shape[0] * per)
        if name.endswith("boundary"):
            assert (shape[0] + 1) * per == LG.LIMIT, name
    for shape in (LG.HALO_F16, LG.HALO_SPLIT):   # the dense halo rows plan onto the big-plane halo kernel (ops.conv3x3_halo would also take CK_HALO_SEG)
        assert LG.dense_halo_plan(shape).kernel == "CK_HALO", shape
    for shape in (LG.GN_SHAPE, LG.ELEMENTWISE_SHAPE):   # elements, not only bytes
        assert shape[0] * shape[1] * shape[2] * shape[3] > LG.G31


# what a dense layer of the grid with x0 in (2^31, limit) bytes plans onto, as (kernel, split-K): the sweep's finding, pinned
DENSE_REACHED = {("CK_HALO", False), ("CK_IGEMM", False), ("CK_IGEMM2", False), ("CK_SPLIT", False)}
CONFIG_REACHED = DENSE_REACHED   # ... and a layer of a shipped config at any batch up to 256
WIDE_ROWS_ONLY = {("CK_IGEMM3", False), ("CK_HALO_SEG", True), ("CK_SPLIT", True)}


def _config_layers():
    """(H, W, Cin, Cout, k, stride, up) of the conv layers of every shipped config (resshift_amd/configs), derived from the YAML: the
    autoencoder's ResnetBlocks (conv1 / conv2 / nin_shortcut), down- and upsampling convs per level at the config's resolution, and the UNet's
    ResBlock, skip and resampling convs per level at its latent size (decoder side: the channel concatenations as one source)"""
    from resshift_amd.config import CONFIG_DIR, load_config, to_plain

    out = set()
    for name in sorted(os.listdir(CONFIG_DIR)):
        cfg = to_plain(load_config(name))
        dd = cfg["autoencoder"]["params"]["ddconfig"] if cfg.get("autoencoder") else None
        if dd:
            ch, mult, res = int(dd["ch"]), [int(v) for v in dd["ch_mult"]], int(dd["resolution"])
            for lvl, m in enumerate(mult):
                r, c = res >> lvl, ch * m
                for cin in {ch * ([1] + mult)[lvl], c, ch * mult[min(lvl + 1, len(mult) - 1)]}:   # encoder entry, same width, decoder entry
                    out |= {(r, r, cin, c, 3, 1, 1), (r, r, cin, c, 1, 1, 1)}
                out |= {(r, r, c, c, 3, 2, 1), (r // 2, r // 2, c, c, 3, 1, 2)}
        mp = cfg["model"]["params"]
        mc, mult, hz = int(mp["model_channels"]), [int(v) for v in mp["channel_mult"]], int(mp["image_size"])
        for lvl, m in enumerate(mult):
            r, c = hz >> lvl, mc * m
            for cin in {mc * ([1] + mult)[lvl], c, 2 * c, c + mc * ([1] + mult)[lvl], c + mc * mult[min(lvl + 1, len(mult) - 1)]}:
                out |= {(r, r, cin, c, 3, 1, 1), (r, r, cin, c, 1, 1, 1)}
            out |= {(r, r, c, c, 3, 2, 1), (r // 2, r // 2, c, c, 3, 1, 2)}
    return sorted(t for t in out if t[0] >= 8)


def test_planner_sweep_over_the_shipped_configs_layers():
    """the same question over the layers of the shipped configs at EVERY batch 1 .. 256: the 256 x 256 and 512 x 512 autoencoder planes are where
    production tensors pass 2^31 bytes.  The kernels reached are the dense grid's, and every one of them has its GPU row"""
    found = {}
    for in_prec, out_prec in CC.STORAGE:
        for Hh, W, Cin, Cout, k, stride, up in _config_layers():
            per = Hh * W * Cin * LG.ESZ[in_prec]
            for B in range(LG.G31 // per + 1, 257):
                if B * per >= LG.LIMIT:
                    break
                p = CC.plan_of(CC.Layer(in_prec, out_prec, B, Hh, W, Cin, Cout, k, stride, up, False))
                if p is not None:
                    found.setdefault((p.kernel, p.splitk > 1), (in_prec, out_prec, B, Hh, W, Cin, Cout, k, stride, up))
    for key in sorted(found):
        print(f"[large] config layer of at least 2^31 bytes on {key}: {found[key]}")
    assert set(found) == CONFIG_REACHED, sorted(found)


def test_planner_sweep_names_the_kernels_a_large_layer_reaches():
    found = {}
    for in_prec, out_prec in CC.STORAGE:
        for k, stride, up in CC.OPS:
            for Hh, W in CC.PLANES:
                for Cin in CC.CIN:
                    per = Hh * W * Cin * LG.ESZ[in_prec]
                    for B in sorted({LG.G31 // per + 1, 256}):   # the smallest batch past 2^31 bytes, and the largest of the grid
                        if B > 256 or not LG.G31 < B * per < LG.LIMIT:
                            continue
                        for Cout in CC.COUT:
                            L = CC.Layer(in_prec, out_prec, B, Hh, W, Cin, Cout, k, stride, up, False)
                            p = CC.plan_of(L)
                            if p is not None:
                                found.setdefault((p.kernel, p.splitk > 1), L)
    for key in sorted(found):
        print(f"[large] dense layer of at least 2^31 bytes on {key}: {tuple(found[key])}")
    assert set(found) == DENSE_REACHED, sorted(found)
    # the rest is reached through wide rows, and has its GPU case (ops.conv_plan cannot ask for the Winograd kernel: its plan needs the
    # packed Winograd weights; ops.conv3x3_wino raises unless that kernel took the launch)
    wide = {(c.kernel, c.sk) for c in LG.CONV_CASES if c.kernel in BUFFER_KERNELS}
    assert WIDE_ROWS_ONLY <= wide, sorted(WIDE_ROWS_ONLY - wide)
    assert DENSE_REACHED | WIDE_ROWS_ONLY >= wide


# ---------------------------------------------------------------- the engine refuses while it plans
def _largest_operand(name, call):
    """elements per image of the largest tensor a buffer-offset conv of the call reads, from the config: the encoder's first level carries
    `ch` channels at the image's resolution throughout; the decoder enters its last level, at that resolution, with the channels of the
    level before it (ldm/modules/diffusionmodules/model.py:589-611: block_in of up level 0's first ResnetBlock is ch * ch_mult[1])"""
    from resshift_amd.config import load_config, to_plain

    dd = to_plain(load_config(name))["autoencoder"]["params"]["ddconfig"]
    mult = 1 if call == "encode" else int(dd["ch_mult"][min(1, len(dd["ch_mult"]) - 1)])
    return int(dd["resolution"]) ** 2 * int(dd["ch"]) * mult


REFUSALS = [("faceir_gfpgan512_lpips", "encode", 2), ("realsr_swinunet_realesrgan256", "encode", 2), ("realsr_swinunet_realesrgan256", "decode", 0)]


@pytest.mark.parametrize("name,call,prec", REFUSALS, ids=[f"{n.split('_')[0]}-{c}-{'split' if p == 2 else 'fp16'}" for n, c, p in REFUSALS])
def test_engine_refuses_an_oversize_operand_in_the_dry_pass(name, call, prec):
    from resshift_amd import build as _b

    per = _largest_operand(name, call) * (2 if prec == 0 else 4)
    refused = -(-LG.LIMIT // per)            # the first batch at which that tensor is LIMIT bytes or more
    args = [f"{name}:{call}:{refused - 1}:{prec}", f"{name}:{call}:{refused}:{prec}"]
    env = dict(os.environ, RS_FAKE_DEVICE="1", RESSHIFT_HIP_LIB=_b.build_testhooks(), **NO_GPU)
    r = subprocess.run([sys.executable, os.path.join(H.ROOT, "tests", "_fake_device_limit.py")] + args, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    lines = {ln.split()[0]: ln for ln in r.stdout.splitlines()}
    print("\n" + "\n".join(lines.values()))
    ok = re.match(r"\S+ rc (-?\d+) launches (\d+) err (.*)$", lines[args[0]])
    no = re.match(r"\S+ rc (-?\d+) launches (\d+) err (.*)$", lines[args[1]])
    # one below: both passes walk, and the call ends with the fake device's own failure
    assert int(ok.group(1)) == -1 and int(ok.group(2)) > 0 and "launch failed" in ok.group(3) and "operand" not in ok.group(3), lines[args[0]]
    assert re.search(r"^case " + re.escape(args[0]) + r"\n\[fake device\] dry: ", r.stderr, re.M), r.stderr[-1500:]
    # at the limit: refused by name while planning, nothing launched, the real pass never starts
    text = no.group(3)
    assert int(no.group(1)) == -7 and int(no.group(2)) == 0, lines[args[1]]
    assert "operand x0 of " in text and f"is {refused * per} bytes" in text and str(LG.LIMIT) in text and text.endswith(f"the largest batch that fits is {refused - 1}"), text
    assert re.match(r"(enc|dec)\.\S*conv 3x3 \d+->\d+: ", text), text
    assert not re.search(r"^case " + re.escape(args[1]) + r"\n\[fake device\] dry: ", r.stderr, re.M), r.stderr[-1500:]

"""Every plan class of the conv planner, on the kernel it names, against float64.

tests/_conv_classes.py holds one layer per class of rs_conv_plan's decision (storage pair, kernel, pixel tile, channel tile, small-plane
segment, split-K bucket, statistics) over a grid of model-like layers - 227 classes, of which test_conv_igemm, test_conv_igemm2_large and
test_conv_igemm_split reached 54, none of the 39 fp16 -> fp32 ones - and one per (storage pair, kernel, split-K yes/no,
ragged M, ragged N, ragged K slice) combination (88; those tests reached 23).  292 distinct layers, none above 10.4 G multiply-adds.  Each row here:
  * runs through ops.conv2d(..., return_plan=True) and asserts that the plan the launch EXECUTED is the row's, field for field;
  * is compared with float64 F.conv2d of the same operation (nearest x2 first where up == 2; fp16 storage on operands rounded to fp16 first),
    at the tolerances of tests/test_ops_gpu.py by storage: TOL[float16] for fp16 results, TOL_SPLIT for split-storage operands, TOL[float32]
    for fp32 results of fp16 / fp32 operands (fp16 -> fp32 launches accumulate exact fp16 products in fp32, as the fp32-storage kernels do, and
    round no result).  Layers under 1 G multiply-adds have their reference on the CPU, larger ones as float64 F.unfold + matmul on the device;
    test_the_two_references_agree holds the two together at 1e-12;
  * (edge rows) runs once more as its strided twin: the same layer WITH a residual, every operand a view into a wider buffer - ld0 = C0 + 8,
    ldy = Cout + 8, ldres = Cout + 16: the same plan, padding columns of the source and of the residual filled with 1e4, padding columns of
    y (and one whole image behind it) pre-filled with a bit pattern that must survive.  The tables' own rows carry no residual (the planner
    asks of one only that ldres be a multiple of 8, so the residual-free layer wins every tie), and the dense launches above run without:
    the twins are where every kernel's and the split-K reduce's residual path, and ldres, are run - 76 of the 88; the 12 split -> fp32
    twins stay without, because that pair defines no residual (twin_layer);
  * (split-K classes) must be no further from float64 than the class's no-split neighbour (same kernel, BP, BC) plus 2 x the error of torch
    float32 on that layer: the reduce only reorders an fp32 sum.  The eight split-K classes of the halo kernel's four-images-per-tile geometry
    (CK_HALO_SEG, SEG 8) never run without split-K on the grid; their neighbour is the same kernel on its big-plane geometry (CK_HALO), same
    tile, which the tables hold in split storage for both channel tiles.

fp16 results enter the split-K comparison without their final rounding (_rel_beyond_rounding).  With the plain max-norm error the comparison
is between two layers' rounding luck - 2.94e-4 against 2.85e-4 of the largest magnitude, where float32's whole error is 4e-7 - and 13 fp16
classes exceed that bound by up to 1.272 x on kernels that are right (the test prints both ratios under -s; outside fp16 -> fp16 the two are
the same number); what the reduce can change is the fp32 accumulator, and that is what is compared.

Measured on the MI355X: all 548 cases pass in 6.3 s (the file's whole pytest run; tests/test_ops_gpu.py took 17.7 s at the parent commit).  The
worst error is 0.26 of its tolerance (split-storage halo rows; fp16 -> fp32 rows stay below 0.03 of TOL[float32]).  Worst split-K ratio
err / (neighbour + 2 x float32) over the 167 classes: 0.567 (fp32 igemm_kernel 64 x 64, split-K 2, 1x8x8 64 -> 16, 3x3 stride 2); among fp16
results 0.191; among the halo small-plane classes 0.237.

Three mutants, one build each, never committed, arithmetic or in-row indexing only ("before": the conv and epilogue cases of
tests/test_ops_gpu.py and tests/test_ops_regimes_gpu.py as they were, 116 cases; for (c) also the block tests):
(a) the last K slice of igemm2's split-K drops its final stage when the stage count is no multiple of the slice count.  Before:
    test_conv_igemm[case0-dtype0] and [case5-dtype0] (fp16, 23 stages in 2 slices), 2 of 116.  Now also 8 cases here: the four fp16 -> fp16 and
    fp16 -> fp32 rows with 23 stages in 2 slices (1x8x8 160 -> 128, 3x3 stride 1 and 2) and their strided twins.
(b) igemm3's fp32-output epilogue adds the bias twice.  Before: none of 116 (no test ran igemm3 with an fp32 result).  Now: all three
    fp16 -> fp32 igemm3 rows and their two strided twins, 5 cases.
(c) igemm_split's ragged channel tile stores up to the row's stride instead of Cout - n0 columns.  Before: none of 116, and none of the 63
    block cases of test_unet_blocks_gpu.py / test_ae_blocks_gpu.py (a dense y has no padding to write into).  Now: the four strided twins of
    the split-storage rows with Cout = 16 on the 64-channel tile (split and fp32 results, 1x1 and 3x3 stride 2): their sentinels are gone.
"""
import functools
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

import _conv_classes as CC
from test_ops_gpu import TOL, TOL_SPLIT

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(bool(CC.planner_env()), reason=f"planner knobs set in the environment: {CC.planner_env()}")]
torch.set_grad_enabled(False)

CPU_REFERENCE_BELOW = 10 ** 9      # multiply-adds
PAD_X, PAD_Y, PAD_RES = 8, 8, 16   # extra columns of the strided twin's buffers: multiples of 8, so every 16-byte rule of the planner holds
LOUD = 1e4                         # what the padding columns of the sources hold
SENTINEL = {2: 0x7BCD, 4: 0x7F8BCDEF}   # bit patterns of y's padding, per element size (fp16; fp32 and split storage)

CLASS_ROWS = CC.rows(CC.REPRESENTATIVES)
EDGE_ROWS = CC.rows(CC.EDGE_REPRESENTATIVES)
ALL_ROWS = list(dict.fromkeys(CLASS_ROWS + EDGE_ROWS))


def _tol(L):
    if L.in_prec == CC.SPLIT:
        return TOL_SPLIT
    return TOL[torch.float16] if L.out_prec == CC.F16 else TOL[torch.float32]


def _operands(L):
    """unit randn input, weights / sqrt(K), bias, residual - fp32 on the CPU, the storage's rounding applied where it rounds (fp16)"""
    g = torch.Generator().manual_seed(zlib.crc32(repr(tuple(L)).encode()))
    Ho, Wo = CC.out_hw(L)
    x = torch.randn(L.B, L.Cin, L.H, L.W, generator=g)
    w = torch.randn(L.Cout, L.Cin, L.k, L.k, generator=g) / math.sqrt(L.Cin * L.k * L.k)
    b = torch.randn(L.Cout, generator=g)
    r = torch.randn(L.B, L.Cout, Ho, Wo, generator=g) if L.res else None
    if L.in_prec == CC.F16:
        x, w = x.half().float(), w.half().float()
    if r is not None and L.out_prec == CC.F16:
        r = r.half().float()
    return x, w, b, r


def reference(L, x, w, b, r, dtype, device):
    """conv (+ bias, + residual) of the layer in `dtype` on `device`, NCHW: F.conv2d on the CPU, F.unfold + matmul image by image on a GPU"""
    x, w, b = x.to(device, dtype), w.to(device, dtype), b.to(device, dtype)
    if L.up == 2:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    pad = L.k // 2
    if device.type == "cpu":
        y = F.conv2d(x, w, b, stride=L.stride, padding=pad)
    else:
        Ho, Wo = CC.out_hw(L)
        wm = w.reshape(L.Cout, -1)
        y = torch.stack([(wm @ F.unfold(x[i:i + 1], L.k, padding=pad, stride=L.stride)[0]).view(L.Cout, Ho, Wo) for i in range(L.B)])
        y = y + b.view(1, -1, 1, 1)
    return y if r is None else y + r.to(device, dtype)


def _rel(got, ref):
    """max |got - ref| / max |ref|, in float64 where ref lives"""
    return ((got.to(ref.device, torch.float64) - ref).abs().max() / (ref.abs().max() + 1e-12)).item()


def _rel_beyond_rounding(got16, ref):
    """_rel of an fp16 result with the final rounding taken out: |got - ref| less half the spacing of fp16 numbers at got, floored at 0.  What is
    left is the accumulator's distance from float64 - the quantity a split-K reduce can change; the rounding itself is up to 2^-12 of each
    element, a thousand times that, and differs from layer to layer by chance."""
    got = got16.to(ref.device, torch.float64)
    half_spacing = torch.ldexp(torch.ones_like(got), (torch.frexp(got)[1] - 12).clamp(min=-25))
    return (((got - ref).abs() - half_spacing).clamp(min=0).max() / (ref.abs().max() + 1e-12)).item()


def _store(t_nchw, prec, dev, pad=0):
    """fp32 NCHW (CPU) -> NHWC device tensor in storage `prec`, `pad` more columns of LOUD behind the channels"""
    from resshift_amd import ops

    t = t_nchw.permute(0, 2, 3, 1)
    if pad:
        t = torch.cat([t, torch.full((*t.shape[:3], pad), LOUD)], 3)
    t = t.contiguous().to(dev)
    return t.half() if prec == CC.F16 else ops.convert(t, ops.SPLIT) if prec == CC.SPLIT else t


def _bits(y):
    """integer view of a stored tensor whose last axis runs over its row's elements: [..., ld] (fp16, fp32) or [..., 2, ld] (split: hi | lo)"""
    if y.dtype == torch.int32:
        return y.view(torch.int16).view(*y.shape[:-1], 2, y.shape[-1])
    return y.view(torch.int16 if y.dtype == torch.float16 else torch.int32)


def _load(y, prec, Cout):
    """stored NHWC result [..., ldy] -> fp32 NCHW of its first Cout columns"""
    from resshift_amd import ops

    y = ops.convert(y, ops.F32) if prec == CC.SPLIT else y
    return y[..., :Cout].permute(0, 3, 1, 2)


def twin_layer(L):
    """the layer a row's strided twin runs: the row's with a residual.  Split -> fp32 launches stay without: there the kernel reads a residual
    as split storage and the split-K reduce reads it as fp32, so the pair defines none (the model's fp32 heads have no shortcut)"""
    return L if (L.in_prec, L.out_prec) == (CC.SPLIT, CC.F32) else L._replace(res=True)


@functools.lru_cache(maxsize=None)
def measure(L, strided=False):
    """one launch of the layer: the executed plan, its error against float64 (relative to the reference's largest magnitude) and, for the
    dense launch, torch float32's error on the same operands; strided: the layer with a residual (twin_layer), every operand a view into a
    wider buffer, and also whether the padding of y survived.  Numbers only are kept."""
    from resshift_amd import ops

    dev = torch.device("cuda:0")
    if strided:
        L = twin_layer(L)
    x, w, b, r = _operands(L)
    ref_dev = torch.device("cpu") if CC.cost(L) < CPU_REFERENCE_BELOW else dev
    ref = reference(L, x, w, b, r, torch.float64, ref_dev)
    Ho, Wo = CC.out_hw(L)
    px, py, pr = (PAD_X, PAD_Y, PAD_RES) if strided else (0, 0, 0)
    xd = _store(x, L.in_prec, dev, px)
    rd = _store(r, L.out_prec, dev, pr) if r is not None else None
    out = {}
    if strided:
        # y's buffer with one more image behind it: the launch gets the first B images, every column past Cout and the whole last image must
        # come back as they were
        backing = torch.empty(L.B + 1, Ho, Wo, L.Cout + py, device=dev, dtype=ops._dt(L.out_prec))
        esz = 2 if L.out_prec == CC.F16 else 4
        backing.view(torch.int16 if esz == 2 else torch.int32).fill_(SENTINEL[esz])
        before_pad, before_tail = _bits(backing[:L.B])[..., L.Cout:].clone(), _bits(backing[L.B:]).clone()
        y, plan = ops.conv2d(xd, w, b, res=rd, stride=L.stride, pad=(L.k // 2, L.k // 2), up=L.up, out_prec=L.out_prec,
                             ld=(L.Cin + px, L.Cout + py, L.Cout + pr), return_plan=True, out=backing[:L.B])
        torch.cuda.synchronize()
        out["intact"] = bool(torch.equal(_bits(backing[:L.B])[..., L.Cout:], before_pad) and torch.equal(_bits(backing[L.B:]), before_tail))
    else:
        y, plan = ops.conv2d(xd, w, b, res=rd, stride=L.stride, pad=(L.k // 2, L.k // 2), up=L.up, out_prec=L.out_prec, return_plan=True)
        torch.cuda.synchronize()
        assert tuple(y.shape) == (L.B, Ho, Wo, L.Cout)
        if plan.splitk > 1:
            out["err32"] = _rel(reference(L, x, w, b, r, torch.float32, ref_dev), ref)
    out["plan"] = CC.Plan(*plan)
    out["err"] = _rel(_load(y, L.out_prec, L.Cout), ref)
    out["acc_err"] = _rel_beyond_rounding(_load(y, L.out_prec, L.Cout), ref) if L.out_prec == CC.F16 else out["err"]
    return out


def _ids(rows):
    return [CC.row_id(L, p) for L, p in rows]


@pytest.mark.parametrize("L,plan", ALL_ROWS, ids=_ids(ALL_ROWS))
def test_row_runs_its_plan_and_matches_float64(gpu, L, plan):
    m = measure(L)
    print(f"\n[conv plan] {CC.row_id(L, plan)}: {CC.cost(L) / 1e9:.2f} G multiply-adds, err {m['err']:.3e} (tol {_tol(L):.0e})")
    assert m["plan"] == plan, (m["plan"], plan)
    assert math.isfinite(m["err"]) and m["err"] <= _tol(L), f"max abs err {m['err']:.3e} of the reference's max (tol {_tol(L)})"


@pytest.mark.parametrize("L,plan", EDGE_ROWS, ids=_ids(EDGE_ROWS))
def test_strided_twin(gpu, L, plan):
    m = measure(L, True)
    print(f"\n[conv plan] strided {CC.row_id(twin_layer(L), plan)}: err {m['err']:.3e} (tol {_tol(L):.0e}), padding intact: {m['intact']}")
    assert m["plan"] == plan, (m["plan"], plan)
    assert m["intact"], "the launch wrote into y's padding columns or behind its last row"
    assert math.isfinite(m["err"]) and m["err"] <= _tol(L), f"max abs err {m['err']:.3e} of the reference's max (tol {_tol(L)})"


def _neighbour(L, p):
    """the first no-split row of the tables on the same kernel, storage pair and tile.  The halo kernel's small-plane geometry (CK_HALO_SEG)
    never runs without split-K on the grid: its neighbour is the same kernel (igemm4.hip) on the big-plane geometry, CK_HALO, same tile"""
    kernel = "CK_HALO" if p.kernel == "CK_HALO_SEG" else p.kernel
    for L2, p2 in ALL_ROWS:
        if (L2.in_prec, L2.out_prec, p2.kernel, p2.BP, p2.BC, p2.splitk) == (L.in_prec, L.out_prec, kernel, p.BP, p.BC, 1):
            return L2
    return None


SPLITK_ROWS = [(L, p) for L, p in CLASS_ROWS if p.splitk > 1]
PAIRED = [(L, p, _neighbour(L, p)) for L, p in SPLITK_ROWS]   # (a class without a neighbour fails its case)


@pytest.mark.parametrize("L,plan,near", PAIRED, ids=_ids([r[:2] for r in PAIRED]))
def test_splitk_is_no_worse_than_its_no_split_neighbour(gpu, L, plan, near):
    """errors as `measure` has them; fp16 results less their final rounding (_rel_beyond_rounding), which the reduce does not touch.  The
    same figures with that rounding left in are printed beside them."""
    assert near is not None, "no no-split row of this kernel and tile in the tables"
    m, n = measure(L), measure(near)
    bound = n["acc_err"] + 2.0 * m["err32"]
    print(f"\n[conv plan] split-K {CC.row_id(L, plan)}: err {m['acc_err']:.3e}, neighbour {n['acc_err']:.3e}, float32 {m['err32']:.3e}, "
          f"ratio to the bound {m['acc_err'] / bound:.3f}; with the stored results' rounding left in: err {m['err']:.3e}, neighbour "
          f"{n['err']:.3e}, ratio {m['err'] / (n['err'] + 2.0 * m['err32']):.3f}")
    assert m["plan"] == plan and n["plan"].splitk == 1
    assert m["acc_err"] <= bound, (m["acc_err"], n["acc_err"], m["err32"])


def test_the_two_references_agree(gpu):
    """float64 F.conv2d on the CPU and float64 F.unfold + matmul on the device: one small layer of each op of the grid, with a residual"""
    for k, stride, up in CC.OPS:
        L = CC.Layer(CC.F32, CC.F32, 3, 12, 10, 24, 40, k, stride, up, True)
        x, w, b, r = _operands(L)
        a = reference(L, x, w, b, r, torch.float64, torch.device("cpu"))
        d = reference(L, x, w, b, r, torch.float64, gpu)
        assert a.shape == d.shape and _rel(d, a) <= 1e-12, (L, _rel(d, a))

"""Per-kernel parity off the unit-scale regime: activation epilogues over their whole range, peaked softmaxes, eps-dominated GroupNorm.

tests/test_ops_gpu.py feeds every kernel unit-scale randn: no GELU or SiLU argument beyond |x| ~ 6, no softmax row with a dominant entry,
no GroupNorm variance within four orders of magnitude of eps.  The model-level tests load one weight draw with the same ranges.  Here the
same kernels, at their smallest shapes, get the operands of the "loud" and "quiet" weight regimes (oracle/synth.py: regime_state_dict):
relative position bias table x 8, qkv weights x 3 or q, k x 4, fc1 scaled until the hidden pre-activations reach +-30, GroupNorm inputs
whose variance is eps or a hundredth of it.  References are float64.  fp16-storage kernels are compared on operands rounded first, with
the tolerances of tests/test_ops_gpu.py; fp32 and split kernels with max(that tolerance, k * err32), err32 the error of torch float32 on
the same formula against float64 (k = 4 for fp32 storage, 8 for split: tests/_regimes.py).  Every softmax case asserts that its
reference's median largest probability is >= 0.5, so the case is what it claims.

Three arithmetic-only mutants were tried against these tests and the regime cases of the block tests, one build each, never committed
(MI355X; "before" = the tests the suite had before the regimes):
1. The autoencoder's GroupNorm eps 1e-6 -> 1e-5 at the four places the graph sets it (csrc/graphs.h: resnet, the attention norm, both heads).
   Before: test_groupnorm / test_groupnorm_split cannot see it (eps is their argument: 76 passed).  Of the base autoencoder block cases at
   B <= 3 (11 cases) the five in split storage notice it, by a factor 2.6 at most (1.3e-5 against 5e-6: the smallest variance of the
   draw is 1e5 eps); the six in fp16 storage - the parity policy's decoder - pass.  Now: all five quiet autoencoder block cases fail,
   fp16 included, by errors of 0.06 .. 0.87 against 5e-6 / 1e-5 / 2.5e-3.
2. rs_gelu_fast's clamp 4.6 -> 3.0 (csrc/common.h).  Before: test_swin_mlp_fused passes (4 cases).  Now:
   test_activation_epilogue_over_the_whole_range[fp16-gelu] fails on 7559 of 8192 elements, by up to 1230 x its bound (|err| 6.2e-3 at
   x = -4.59; -0.047 at x = -34.6, where the result must be -0; 0.14 at most);test_swin_mlp_fused_over_the_gelu_range[fp16] does not see it through fc2's
   max-norm (3.4e-4 of 2e-3), which is why the epilogue is checked element by element.
3. The row maximum replaced by 0 in win_attn_qkv_split_kernel's softmax (csrc/win_attn_split.hip).  Before:
   test_window_attention_fused_qkv_split passes (5 cases: no logit leaves +-10, exp2 does not overflow).  Now: all three
   test_window_attention_fused_qkv_split_peaked cases and the loud split UNet block case fail with NaN outputs.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import _regimes as R
from test_ops_gpu import _close, _nhwc, _ref_in, _split, _unsplit, _window_attention_reference

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

STORAGES = ("fp16", "split", "fp32")
U = {"fp16": 2.0 ** -11, "split": 2.0 ** -22, "fp32": 2.0 ** -23}     # relative rounding of the stored result
# the smallest step of the stored result near zero: half an fp16 subnormal step; the split pair's floor (lo is kept scaled by 2^11:
# test_split_storage_roundtrip); the smallest normal fp32 number (subnormal results may be flushed)
B_STORE = {"fp16": 2.0 ** -25, "split": 2.0 ** -35, "fp32": 2.0 ** -126}


def _rel(got, ref):
    """max |got - ref| / max |ref|"""
    return ((got.double() - ref).abs().max() / ref.abs().max()).item()


def _tol(prec, existing, ref32, ref64):
    """max(existing, k * err32) for fp32 / split storage, err32 = torch float32 of the same formula against float64; fp16 keeps `existing`"""
    k = R.K32.get(prec)
    return existing if k is None else max(existing, k * _rel(ref32, ref64))


def _peaked(p):
    assert p.finite and p.median_pmax() >= 0.5, f"not a peaked case: median largest probability {p.median_pmax():.3f}"
    return p.median_pmax()


# ---------------------------------------------------------------- activation epilogues over the whole range
def _act_bound(prec, act, x):
    """(a [per element], b) of |err| <= u |ref| + a |x| + b for the form of `act` that storage `prec` gets (csrc/igemm_common.h: fp16 outputs
    take the rs_*_fast forms, fp32 and split outputs rs_gelu / rs_silu), from what the comments in csrc/common.h state:

    rs_gelu_fast - "erf(x / sqrt 2) ~= x P(x^2) / Q(x^2) ... on |x| <= 4.6 ... max abs error 1.7e-6; beyond the clamp 1 - erf < 4.2e-6": GELU
        is x/2 (1 + g), so a = 1.7e-6 / 2 up to the clamp and (1.7e-6 + 4.2e-6) / 2 beyond it (the fit's value at the clamp stands in for
        erf(x / sqrt 2)); evaluating g in fp32 - two Horner chains of three FMAs, two products, "v_rcp_f32 ... (1 ulp ...)" - adds at
        most 8 roundings of 2^-24 on |g| <= 1: a += 2^-22.
    rs_gelu (the libm form, "exact-erf GELU"; igemm_split.hip: "exact fp32 arithmetic (IEEE division, libm erff)"): erff within a few ulp
        (2^-24 next to 1) and the rounding of its argument leave 1 + erf good to 4 * 2^-24 absolute - it cancels in the negative tail, in
        torch's float32 GELU as well - times |x| / 2: a = 2^-23.
    rs_silu_fast / rs_silu - "v_rcp_f32 / v_exp_f32 (1 ulp each)" (rs_silu: __expf and the IEEE division): y = x s(x), s = 1 / (1 + e);
        e carries its own ulp and the rounding of its argument, |x| 2^-24 relative, and the add and the reciprocal one more each:
        |err| <= 3 * 2^-23 |y| + 2^-24 x^2 s (1 - s).  |y| <= |x| gives a = 2^-22 on top of u |ref|; x^2 s (1 - s) <= 0.44 gives b = 2^-25.
        Where e^-x overflows fp32 (x < -88.72) the result is -0 and the true value below 104 e^-88.72 < 2^-121, far inside b.
    rs_gelu_acc and rs_silu_acc ("good to ~3e-7 of |x| + 1.5e-7") have no caller; rs_gelu_acc2 is the hidden activation of the fused split
        MLP, which no output shows directly: test_swin_mlp_fused_over_the_gelu_range checks it through fc2 in the existing max-norm."""
    ax = x.abs().double()
    if act == "gelu" and prec == "fp16":
        a = torch.where(ax <= 4.6, 0.5 * 1.7e-6, 0.5 * (1.7e-6 + 4.2e-6)) + 2.0 ** -22
        return a, B_STORE[prec]
    if act == "gelu":
        return torch.full_like(ax, 2.0 ** -23), B_STORE[prec]
    return torch.full_like(ax, 2.0 ** -22), 2.0 ** -25 + B_STORE[prec]


def _neighbours(v, dtype):
    """v rounded to `dtype` and its two neighbours on either side there, as float32"""
    t = torch.tensor([v], dtype=dtype)
    bits = t.view(torch.int16 if dtype == torch.float16 else torch.int32)
    return torch.cat([(bits + d).view(dtype).float() for d in (-2, -1, 0, 1, 2)])


def _act_inputs(prec, n):
    """n float32 values, each exact in storage `prec`: a grid over [-40, 40] and the points where a form changes branch or an exp
    overflows: +-0, the clamp of the fast GELU +-4.6 with two ulps (fp16's and fp32's) on either side, +-6, -88, -90, -104"""
    special = [torch.tensor([0.0, -0.0, 6.0, -6.0, -88.0, -90.0, -104.0])]
    for s in (4.6, -4.6):
        special += [_neighbours(s, torch.float16), _neighbours(s, torch.float32)]
    special = torch.cat(special)
    x = torch.cat([special, torch.linspace(-40.0, 40.0, n - special.numel())])
    if prec == "fp16":
        return x.half().float()
    if prec == "split":   # hi + lo 2^-11 with fp16 hi and lo: what the pair holds of x, exact in fp32 (11 + 1 + 11 bits)
        hi = x.half().float()
        return hi + ((x - hi) * 2048.0).half().float() / 2048.0
    return x


@pytest.mark.parametrize("act", ["gelu", "silu"])
@pytest.mark.parametrize("prec", STORAGES)
def test_activation_epilogue_over_the_whole_range(gpu, prec, act):
    """ops.conv2d, 1 x 1, identity weight (the accumulator is the input, exactly), C = 64, 128 pixels, GELU / SiLU in the epilogue,
    against float64, element by element: |err| <= u |ref| + a |x| + b (_act_bound)."""
    from resshift_amd import ops

    C, npx = 64, 128
    x = _act_inputs(prec, C * npx)
    x = x[torch.randperm(x.numel(), generator=torch.Generator().manual_seed(3))].view(1, 8, 16, C)   # every value in some lane and row
    w = torch.eye(C).view(C, C, 1, 1)
    xd = x.to(gpu)
    xd = xd.half() if prec == "fp16" else (ops.convert(xd, ops.SPLIT) if prec == "split" else xd)
    if prec == "split":
        assert torch.equal(ops.convert(xd, ops.F32).cpu(), x)    # the inputs are exact in the pair
    y = ops.conv2d(xd, w, None, pad=(0, 0), act=1 if act == "gelu" else 2)
    torch.cuda.synchronize()
    got = (ops.convert(y, ops.F32) if prec == "split" else y).float().cpu().double()
    xv = x.double()
    ref = F.gelu(xv) if act == "gelu" else F.silu(xv)
    a, b = _act_bound(prec, act, x)
    err, bound = (got - ref).abs(), U[prec] * ref.abs() + a * xv.abs() + b
    assert bool(torch.isfinite(got).all())
    worst = (err / bound).max().item()
    i = (err / bound).argmax()
    print(f"\n{act} {prec}: worst |err| / bound {worst:.3f} at x = {xv.view(-1)[i].item():.6g} (err {err.view(-1)[i].item():.3e}); largest |err| {err.max().item():.3e}")
    bad = err > bound
    assert not bad.any(), (int(bad.sum()), xv[bad][:6].tolist(), got[bad][:6].tolist(), ref[bad][:6].tolist())


@pytest.mark.parametrize("prec", ["fp16", "split"])
def test_swin_mlp_fused_over_the_gelu_range(gpu, prec):
    """ops.swin_mlp (swin_mlp.hip: fc1 + GELU + fc2 + shortcut in one launch) at M = 64 with fc1 scaled until the hidden pre-activations
    reach +-30 (rs_gelu_fast past its clamp in fp16, rs_gelu_acc2 with exp(-x^2 / 2) underflowing in split), in the max-norm tolerances of
    test_swin_mlp_fused (2e-3, the hidden activations rounded to fp16 on both sides) and test_swin_mlp_fused_split (3e-6 against float64)."""
    from resshift_amd import ops

    M, E, HD = 64, 192, 768
    g = torch.Generator().manual_seed(64)
    x = torch.randn(M, E, generator=g)
    w1 = torch.randn(HD, E, generator=g) / math.sqrt(E) * 8.0
    w2 = torch.randn(E, HD, generator=g) / math.sqrt(HD)
    b1, b2 = torch.randn(HD, generator=g) * 0.3, torch.randn(E, generator=g) * 0.3
    res = torch.randn(M, E, generator=g)
    if prec == "fp16":
        xd, rd, w1, w2 = x.to(gpu, torch.float16), res.to(gpu, torch.float16), w1.half(), w2.half()
        y = ops.swin_mlp(xd, w1, b1, w2, b2, rd)
        torch.cuda.synchronize()
        pre = xd.double().cpu() @ w1.double().t() + b1.double()
        ref = F.gelu(pre).half().double() @ w2.double().t() + b2.double() + rd.double().cpu()
        got, tol = y.float().cpu(), 2e-3
    else:
        y = ops.convert(ops.swin_mlp(ops.convert(x.to(gpu), ops.SPLIT), w1, b1, w2, b2, ops.convert(res.to(gpu), ops.SPLIT)), ops.F32)
        torch.cuda.synchronize()
        pre = x.double() @ w1.double().t() + b1.double()
        ref = F.gelu(pre) @ w2.double().t() + b2.double() + res.double()
        got, tol = y.cpu(), 3e-6
    assert pre.max().item() >= 30.0 and pre.min().item() <= -30.0, (pre.min().item(), pre.max().item())
    print(f"\nswin mlp {prec}: hidden pre-activations {pre.min().item():.1f} .. {pre.max().item():.1f}, error {_rel(got, ref):.3e} (tolerance {tol:.0e})")
    _close(got, ref, tol, f"swin mlp over the GELU range, {prec}")


# ---------------------------------------------------------------- peaked softmax
WIN = [((8, 8), 0), ((16, 16), 4)]
WIN_IDS = ["8x8-shift0", "16x16-shift4"]


@pytest.mark.parametrize("prec", STORAGES)
@pytest.mark.parametrize("hw,shift", WIN, ids=WIN_IDS)
def test_window_attention_peaked(gpu, prec, hw, shift):
    """test_window_attention / test_window_attention_split with qkv x 3 and the bias table x 8"""
    from resshift_amd import ops

    H, W = hw
    heads = 6
    g = torch.Generator().manual_seed(H * 7 + shift)
    qkv = torch.randn(2, 3 * heads * 32, H, W, generator=g) * 3.0
    table = torch.randn(225, heads, generator=g) * 0.5 * 8.0
    if prec == "split":
        qd, qr = _split(qkv, gpu), qkv
    else:
        qd = _nhwc(qkv, torch.float16 if prec == "fp16" else torch.float32, gpu)
        qr = _ref_in(qd)
    with R.probe() as p:
        ref = _window_attention_reference(qr.double(), table.double(), heads, shift)
    pm = _peaked(p)
    tol = _tol(prec, {"fp16": 2e-3, "fp32": 2e-5, "split": 5e-6}[prec], _window_attention_reference(qr, table, heads, shift), ref)
    out = ops.window_attention(qd, table, heads, shift)
    torch.cuda.synchronize()
    got = (_unsplit(out) if prec == "split" else out.float().cpu()).permute(0, 3, 1, 2)
    print(f"\nwindow attention {prec} {hw} shift {shift}: median largest probability {pm:.3f}, error {_rel(got, ref):.3e} (tolerance {tol:.2e})")
    _close(got, ref, tol, f"peaked window attention {prec} {hw} shift {shift}")


@pytest.mark.parametrize("hw,shift", WIN, ids=WIN_IDS)
def test_window_attention_fused_qkv_peaked(gpu, hw, shift):
    """test_window_attention_fused_qkv with the qkv weights x 3 and the bias table x 8"""
    from resshift_amd import ops

    H, W = hw
    heads, E = 6, 192
    g = torch.Generator().manual_seed(H * 11 + shift)
    x = torch.randn(2, E, H, W, generator=g)
    wqkv = (torch.randn(3 * E, E, generator=g) / math.sqrt(E) * 3.0).half()
    bqkv = torch.randn(3 * E, generator=g) * 0.2
    table = torch.randn(225, heads, generator=g) * 0.5 * 8.0
    xd = _nhwc(x, torch.float16, gpu)
    qkv = torch.einsum("bchw,oc->bohw", _ref_in(xd).double(), wqkv.double()) + bqkv.double()[None, :, None, None]
    with R.probe() as p:
        ref = _window_attention_reference(qkv.half().double(), table.double(), heads, shift)   # qkv rounded to fp16, as the kernel's operands are
    pm = _peaked(p)
    out = ops.window_attention_qkv(xd, wqkv, bqkv, table, heads, shift)
    torch.cuda.synchronize()
    print(f"\nfused qkv window attention {hw} shift {shift}: median largest probability {pm:.3f}, error {_rel(out.float().cpu().permute(0, 3, 1, 2), ref):.3e}")
    _close(out.permute(0, 3, 1, 2), ref, 3e-3, f"peaked fused qkv window attention {hw} shift {shift}")
    wproj = (torch.randn(E, E, generator=g) / math.sqrt(E)).half()
    bproj = torch.randn(E, generator=g) * 0.2
    rd = _nhwc(torch.randn(2, E, H, W, generator=g), torch.float16, gpu)
    ref2 = torch.einsum("bchw,oc->bohw", ref.half().double(), wproj.double()) + bproj.double()[None, :, None, None] + _ref_in(rd).double()
    out2 = ops.window_attention_qkv(xd, wqkv, bqkv, table, heads, shift, wproj=wproj, bproj=bproj, res=rd)
    torch.cuda.synchronize()
    _close(out2.permute(0, 3, 1, 2), ref2, 3e-3, f"peaked fused qkv + proj window attention {hw} shift {shift}")


@pytest.mark.parametrize("hw,shift,fold", [((8, 8), 0, True), ((16, 16), 4, True), ((16, 16), 4, False)],
                         ids=["8x8-shift0-fold", "16x16-shift4-fold", "16x16-shift4"])
def test_window_attention_fused_qkv_split_peaked(gpu, hw, shift, fold):
    """test_window_attention_fused_qkv_split with the qkv weights x 3 and the bias table x 8: logits past +-100, where a softmax without its
    max subtraction overflows"""
    from resshift_amd import ops

    H, W = hw
    heads, E, B = 6, 192, 2
    g = torch.Generator().manual_seed(H * 13 + shift)
    x = torch.randn(B, E, H, W, generator=g)
    wqkv = torch.randn(3 * E, E, generator=g) / math.sqrt(E) * 3.0
    bqkv = torch.randn(3 * E, generator=g) * 0.2
    table = torch.randn(225, heads, generator=g) * 0.5 * 8.0
    wproj = torch.randn(E, E, generator=g) / math.sqrt(E)
    bproj = torch.randn(E, generator=g) * 0.2
    res = torch.randn(B, E, H, W, generator=g)
    coef = torch.stack([1.0 + 0.3 * torch.randn(B, E, generator=g), 0.2 * torch.randn(B, E, generator=g)], 1) if fold else None   # [B,2,E]

    def formula(dt):
        xn = x.to(dt) * coef[:, 0, :, None, None].to(dt) + coef[:, 1, :, None, None].to(dt) if fold else x.to(dt)
        qkv = torch.einsum("bchw,oc->bohw", xn, wqkv.to(dt)) + bqkv.to(dt)[None, :, None, None]
        attn = _window_attention_reference(qkv, table.to(dt), heads, shift)
        return attn, torch.einsum("bchw,oc->bohw", attn, wproj.to(dt)) + bproj.to(dt)[None, :, None, None] + res.to(dt)

    with R.probe() as p:
        attn, ref2 = formula(torch.float64)
    pm = _peaked(p)
    attn32, ref32 = formula(torch.float32)
    t1, t2 = _tol("split", 5e-6, attn32, attn), _tol("split", 5e-6, ref32, ref2)
    out = ops.window_attention_qkv_split(_split(x, gpu), wqkv, bqkv, table, heads, shift, xcoef=coef)
    torch.cuda.synchronize()
    got = _unsplit(out).permute(0, 3, 1, 2)
    print(f"\nfused split qkv window attention {hw} shift {shift}: median largest probability {pm:.3f}, error {_rel(got, attn):.3e} (tolerance {t1:.2e})")
    _close(got, attn, t1, f"peaked fused split qkv window attention {hw} shift {shift}")
    out2 = ops.window_attention_qkv_split(_split(x, gpu), wqkv, bqkv, table, heads, shift, wproj=wproj, bproj=bproj, res=_split(res, gpu), xcoef=coef)
    torch.cuda.synchronize()
    _close(_unsplit(out2).permute(0, 3, 1, 2), ref2, t2, f"peaked fused split qkv + proj window attention {hw} shift {shift}")


def _ae_attention(q, k, v, bv):
    C = q.shape[-1]
    return torch.bmm((torch.bmm(q, k.transpose(1, 2)) * C ** -0.5).softmax(dim=2), v) + bv


def test_ae_flash_attention_peaked(gpu):
    """test_ae_flash_attention at its smallest shape with q, k x 4: the running maximum of the online softmax jumps by tens between key blocks"""
    from resshift_amd import ops

    nz, T, C = 1, 256, 128
    g = torch.Generator().manual_seed(T + C)
    q = (torch.randn(nz, T, C, generator=g) * 1.5 * 4.0).half()
    k = (torch.randn(nz, T, C, generator=g) * 1.5 * 4.0).half()
    v = torch.randn(nz, T, C, generator=g).half()
    bv = torch.randn(C, generator=g) * 0.3
    with R.probe() as p:
        ref = _ae_attention(q.double(), k.double(), v.double(), bv.double())
    pm = _peaked(p)
    o = ops.ae_flash_attention(q.to(gpu), k.to(gpu), v.to(gpu), bv)
    torch.cuda.synchronize()
    print(f"\nstreaming AE attention: median largest probability {pm:.3f}, error {_rel(o.float().cpu(), ref):.3e}")
    _close(o, ref, 3e-3, "peaked streaming AE attention")


def test_ae_flash_attention_split_peaked(gpu):
    """test_ae_flash_attention_split at its smallest shape with q, k x 4"""
    from resshift_amd import ops

    nz, T, C = 1, 64, 512
    g = torch.Generator().manual_seed(T)
    q = torch.randn(nz, T, C, generator=g) * 1.5 * 4.0
    k = torch.randn(nz, T, C, generator=g) * 1.5 * 4.0
    v = torch.randn(nz, T, C, generator=g)
    bv = torch.randn(C, generator=g) * 0.3
    with R.probe() as p:
        ref = _ae_attention(q.double(), k.double(), v.double(), bv.double())
    pm = _peaked(p)
    tol = _tol("split", 3e-6, _ae_attention(q, k, v, bv), ref)
    o = ops.ae_flash_attention_split(q.to(gpu), k.to(gpu), v.to(gpu), bv)
    torch.cuda.synchronize()
    print(f"\nsplit streaming AE attention: median largest probability {pm:.3f}, error {_rel(_unsplit(o), ref):.3e} (tolerance {tol:.2e})")
    _close(_unsplit(o), ref, tol, "peaked split streaming AE attention")


@pytest.mark.parametrize("ncols", [256, 960, 1028])   # one pass of the 256 x 4 lanes; the 40 x 24 latent's token count; a second pass with a tail
@pytest.mark.parametrize("out", ["fp32", "split", "fp16"])
def test_softmax_rows_peaked(gpu, ncols, out):
    """softmax_rows (the materialised softmax of the autoencoder's row-block attention) on logits of scale 30: fp32 and split outputs in the
    tolerances of test_gemm_nt_batched_and_softmax(_split) (1e-5 / 5e-6), the fp16 output within its own rounding (2^-11 of the largest
    probability, which is ~1) on top of the fp32 output's 1e-5"""
    from resshift_amd import ops

    nrows = 96
    s = torch.randn(nrows, ncols, generator=torch.Generator().manual_seed(ncols)) * 30.0
    s[0] = 0.0            # a flat row
    s[1, 5] = 300.0       # one entry takes everything: every other exp underflows
    with R.probe() as p:
        ref = s.double().softmax(-1)
    pm = _peaked(p)
    tol = _tol(out, {"fp32": 1e-5, "split": 5e-6, "fp16": 2.0 ** -11 + 1e-5}[out], s.softmax(-1), ref)
    y = ops.softmax_rows(s.to(gpu), out_prec={"fp32": ops.F32, "split": ops.SPLIT, "fp16": ops.F16}[out])
    torch.cuda.synchronize()
    got = _unsplit(y) if out == "split" else y.float().cpu()
    print(f"\nsoftmax_rows {ncols} -> {out}: median largest probability {pm:.3f}, error {_rel(got, ref):.3e} (tolerance {tol:.2e})")
    _close(got, ref, tol, f"peaked softmax_rows {ncols} {out}")
    assert ((got.double().sum(-1) - 1.0).abs() <= ncols * U[out]).all()


# ---------------------------------------------------------------- GroupNorm where eps matters
@pytest.mark.parametrize("prec", STORAGES)
@pytest.mark.parametrize("shape", [(1, 16, 16, 64), (2, 16, 16, 160), (1, 64, 64, 128)], ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("mode", ["plain", "film_silu"])
@pytest.mark.parametrize("quiet", ["var~eps", "var<<eps"])
def test_groupnorm_eps_dominated(gpu, prec, shape, mode, quiet):
    """ops.groupnorm with var ~ eps (x = 0.003 randn + 0.003) and var << eps (x = 0.0003 randn): with eps 1e-5 instead of 1e-6 or the
    other way round the output moves by tens of percents here - by 4.5e-6 at var ~ 1.  Tolerances of test_groupnorm / test_groupnorm_split."""
    from resshift_amd import ops

    B, H, W, C = shape
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(B, C, H, W, generator=g) * 0.003 + 0.003 if quiet == "var~eps" else torch.randn(B, C, H, W, generator=g) * 0.0003
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    eps = 1e-5 if mode != "plain" else 1e-6
    if prec == "split":
        xd, xr = _split(x, gpu), x
    else:
        xd = _nhwc(x, torch.float16 if prec == "fp16" else torch.float32, gpu)
        xr = _ref_in(xd)
    ref = F.group_norm(xr.double(), 32, gamma.double(), beta.double(), eps)
    film_d = None
    if mode == "film_silu":
        film = torch.randn(2 * C, generator=g) * 0.5
        film_d = film.to(gpu)
        ref = F.silu(ref * (1 + film[:C].double().view(1, C, 1, 1)) + film[C:].double().view(1, C, 1, 1))
    v = xr.double().reshape(B, 32, -1).var(dim=2, unbiased=False)
    assert (v / eps).max().item() <= (20.0 if quiet == "var~eps" else 0.2)    # eps-dominated, as claimed
    y = ops.groupnorm(xd, gamma, beta, eps, act=0 if mode == "plain" else 2, film=film_d)
    torch.cuda.synchronize()
    got = (_unsplit(y) if prec == "split" else y.float().cpu()).permute(0, 3, 1, 2)
    _close(got, ref, {"fp16": 2e-3, "split": 5e-6, "fp32": 5e-5}[prec], f"eps-dominated groupnorm {prec} {shape} {mode} {quiet}")

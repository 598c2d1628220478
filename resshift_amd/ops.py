"""Thin torch-tensor wrappers over the op-level C-ABI entry points (rs_op_*).

They exist so that tests/ can check every HIP kernel in isolation against a torch fp32 reference.
Tensors are NHWC (channels last, contiguous) on the GPU; `prec` 0 = fp16 storage, 1 = fp32 storage, 2 = split storage
((hi, lo) fp16 pairs, 4 bytes per element: carried in torch.int32 tensors of the logical shape, see `convert`).
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import torch

from . import _lib

F16, F32, SPLIT = _lib.RS_PREC_F16, _lib.RS_PREC_F32, _lib.RS_PREC_SPLIT


def _dt(prec: int) -> torch.dtype:
    return {F16: torch.float16, F32: torch.float32, SPLIT: torch.int32}[prec]


def _prec_of(t: torch.Tensor) -> int:
    return {torch.float16: F16, torch.float32: F32, torch.int32: SPLIT}[t.dtype]


def _out_or_new(out, shape, like):
    """the caller's result tensor (`out=` of the wrappers that take one: contiguous, of the result's shape and the operand's storage), or a new one"""
    if out is None:
        return torch.empty(shape, device=like.device, dtype=like.dtype)
    assert tuple(out.shape) == tuple(shape) and out.dtype == like.dtype and out.is_contiguous()
    return out


def convert(x, prec):
    """Storage conversion of an NHWC tensor [..., C] (fp16 / fp32 / split-as-int32) to `prec`."""
    lib = _lib.load()
    x = x.contiguous()
    Cc = x.shape[-1]
    out = torch.empty(x.shape, device=x.device, dtype=_dt(prec))
    _lib.check(lib.rs_op_convert(x.data_ptr(), _prec_of(x), out.data_ptr(), prec, Cc, x.numel() // Cc, _lib.current_stream_ptr()), "convert")
    return out


def _hostf(t: torch.Tensor):
    t = t.detach().to("cpu", torch.float32).contiguous()
    return t, t.data_ptr()


CONV_KERNELS = ("CK_NONE", "CK_WINO", "CK_HALO", "CK_HALO_SEG", "CK_SPLIT", "CK_IGEMM3", "CK_IGEMM2", "CK_IGEMM")   # enum ConvKernel, csrc/common.h
ConvPlan = namedtuple("ConvPlan", "kernel BP BC SEG splitk stats_px")   # struct ConvPlan (csrc/common.h) with the kernel by name


def _plan(ints):
    return ConvPlan(CONV_KERNELS[ints[0]], *ints[1:6])


def _out_hw(Hs, Ws, KH, KW, stride, pad, up):
    return (Hs * up + 2 * pad[0] - KH) // stride + 1, (Ws * up + 2 * pad[1] - KW) // stride + 1


def conv_plan(B, Hs, Ws, C0, Cout, k, in_prec, out_prec=None, C1=0, stride=1, pad=None, out_hw=None, up=1, act=0, has_res=False, ld=None, nz=1):
    """The plan `conv2d` would execute for this layer (rs_op_conv_plan: host code only, no device): a ConvPlan, or None when no kernel takes
    the launch.  k: the square kernel's size; pad defaults to (k // 2, k // 2); ld = (ld0, ldy, ldres) as `conv2d` takes it.  A layer that
    `conv2d` hands to the direct kernels answers ConvPlan("CK_NONE", 0, 0, 0, 0, 0)."""
    lib = _lib.load()
    out_prec = in_prec if out_prec is None else out_prec
    pad = (k // 2, k // 2) if pad is None else pad
    Ho, Wo = _out_hw(Hs, Ws, k, k, stride, pad, up) if out_hw is None else out_hw
    ld0, ldy, ldres = (C0, Cout, Cout) if ld is None else ld
    out = (C.c_int * 6)()
    rc = lib.rs_op_conv_plan(B, Hs, Ws, C0, C1, Cout, k, k, stride, pad[0], pad[1], Ho, Wo, up, act, in_prec, out_prec, ld0, C1, ldy, ldres,
                             int(has_res), nz, out)
    return None if rc else _plan(out)


def conv2d(x0, w_ref, bias=None, x1=None, res=None, stride=1, pad=(1, 1), out_hw=None, up=1, act=0, out_prec=None,
           force_direct=False, ld=None, return_plan=False, out=None):
    """x0: [B,H,W,C0] (+x1 [B,H,W,C1]); w_ref: reference layout [Cout,Cin,KH,KW]; returns [B,Ho,Wo,Cout].
    ld = (ld0, ldy, ldres): the operands are views into wider buffers and the caller passes those - x0 [B,H,W,ld0] whose first C0 = Cin - C1
    columns are the source, res [B,Ho,Wo,ldres]; y is allocated [B,Ho,Wo,ldy] (or is `out`, of that shape) and returned whole.
    return_plan: returns (y, ConvPlan), the plan the launch executed (all zeros under CK_NONE when a direct kernel took it)."""
    lib = _lib.load()
    in_prec = _prec_of(x0)
    out_prec = in_prec if out_prec is None else out_prec
    C1 = 0 if x1 is None else x1.shape[-1]
    Cout, Cin, KH, KW = w_ref.shape
    B, Hs, Ws, ld0 = x0.shape
    C0 = ld0 if ld is None else Cin - C1
    assert Cin == C0 + C1
    ld0_, ldy, ldres = (C0, Cout, Cout) if ld is None else ld
    assert ld0_ == ld0 and C0 <= ld0 and Cout <= ldy and (res is None or (Cout <= ldres and res.shape[-1] == ldres))
    pad_t, pad_l = pad
    Ho, Wo = _out_hw(Hs, Ws, KH, KW, stride, pad, up) if out_hw is None else out_hw
    y = torch.empty(B, Ho, Wo, ldy, device=x0.device, dtype=_dt(out_prec)) if out is None else out
    assert tuple(y.shape) == (B, Ho, Wo, ldy) and y.dtype == _dt(out_prec) and y.is_contiguous()
    assert res is None or (tuple(res.shape[:3]) == (B, Ho, Wo) and res.is_contiguous())
    wh, wp = _hostf(w_ref)
    bh, bp = _hostf(bias) if bias is not None else (None, None)
    plan = (C.c_int * 6)()
    rc = lib.rs_op_conv2d_ex(x0.data_ptr(), x1.data_ptr() if x1 is not None else None, wp, bp,
                             res.data_ptr() if res is not None else None, y.data_ptr(), B, Hs, Ws, C0, C1, Cout, KH, KW, stride,
                             pad_t, pad_l, Ho, Wo, up, act, in_prec, out_prec, int(force_direct), ld0, C1, ldy, ldres, plan,
                             _lib.current_stream_ptr())
    _lib.check(rc, "rs_op_conv2d_ex")
    return (y, _plan(plan)) if return_plan else y


def conv3x3_halo(x, w_ref, bias=None, coef=None, act_in=0, res=None, want_stats=False):
    """Halo-tile 3x3 conv (igemm4.hip): x [B,H,W,Cin] raw tensor (fp16, or split storage as int32), coef [B,2,Cin] fp32 device
    (GroupNorm affine: scale row, shift row) applied with `act_in` (0 none / 2 SiLU) to x inside the kernel; returns [B,H,W,Cout]
    in the same storage (with `want_stats` also the [B, slabs, Cout, 2] sums / sums of squares of the stored output; a slab is one
    pixel tile of the kernel variant or one reduce-kernel slab)."""
    lib = _lib.load()
    B, H, W, Cin = x.shape
    Cout = w_ref.shape[0]
    prec = _prec_of(x)
    y = torch.empty(B, H, W, Cout, device=x.device, dtype=x.dtype)
    wh, wp = _hostf(w_ref)
    bh, bp = _hostf(bias) if bias is not None else (None, None)
    st = None
    if want_stats:
        spx = lib.rs_op_conv3x3_halo_stats_px(B, H, W, Cin, Cout, prec)
        if spx <= 0:
            raise RuntimeError("this shape gets no output statistics from the halo kernel")
        st = torch.zeros(B, (H * W) // spx, Cout, 2, device=x.device, dtype=torch.float32)
    rc = lib.rs_op_conv3x3_halo(x.data_ptr(), coef.data_ptr() if coef is not None else None, act_in, wp, bp,
                                res.data_ptr() if res is not None else None, y.data_ptr(), B, H, W, Cin, Cout, prec,
                                st.data_ptr() if st is not None else None, _lib.current_stream_ptr())
    _lib.check(rc, "rs_op_conv3x3_halo")
    return (y, st) if want_stats else y


def conv3x3_wino(x, w_ref, bias=None, coef=None, act_in=0, res=None, want_stats=False, reps=0, out=None):
    """Winograd F(2x2,3x3) conv (wino.hip): x [B,H,W,Cin] raw split-storage tensor (int32), coef [B,2,Cin] fp32 device (GroupNorm
    affine) applied with `act_in` (0 none / 2 SiLU) inside the kernel; returns [B,H,W,Cout] in split storage (with `want_stats` also
    the [B, H*W/128, Cout, 2] sums / sums of squares of the stored output; with reps > 0 also the average ms per launch)."""
    lib = _lib.load()
    B, H, W, Cin = x.shape
    Cout = w_ref.shape[0]
    if _prec_of(x) != 2:
        raise RuntimeError("the wino kernel takes split storage")
    y = _out_or_new(out, (B, H, W, Cout), x)
    wh, wp = _hostf(w_ref)
    bh, bp = _hostf(bias) if bias is not None else (None, None)
    st = torch.zeros(B, (H * W) // 128, Cout, 2, device=x.device, dtype=torch.float32) if want_stats else None
    ms = C.c_float(0.0)
    rc = lib.rs_op_conv3x3_wino(x.data_ptr(), coef.data_ptr() if coef is not None else None, act_in, wp, bp,
                                res.data_ptr() if res is not None else None, y.data_ptr(), B, H, W, Cin, Cout,
                                st.data_ptr() if st is not None else None, reps, C.byref(ms), _lib.current_stream_ptr())
    _lib.check(rc, "rs_op_conv3x3_wino")
    out = (y, st) if want_stats else y
    return (out, ms.value) if reps > 0 else out


def gemm_nt(a, b, bias=None, scale=1.0, out_prec=None):
    """a: [nz,M,K], b: [nz,N,K] -> [nz,M,N] = scale * a @ b^T (+bias[n], fp32 device tensor)."""
    lib = _lib.load()
    in_prec = _prec_of(a)
    out_prec = in_prec if out_prec is None else out_prec
    nz, M, K = a.shape
    N = b.shape[1]
    y = torch.empty(nz, M, N, device=a.device, dtype=_dt(out_prec))
    rc = lib.rs_op_gemm_nt(a.data_ptr(), b.data_ptr(), bias.data_ptr() if bias is not None else None, y.data_ptr(), nz, M, N, K,
                           float(scale), in_prec, out_prec, _lib.current_stream_ptr())
    _lib.check(rc, "rs_op_gemm_nt")
    return y


def groupnorm(x, gamma, beta, eps, act=0, film=None, groups=32, out=None):
    """x: [B,H,W,C]; film: optional fp32 device tensor [2C] (scale, shift); out: the result's tensor.  out = x (in place) is for planes above 256 pixels only: there a
    statistics pass ends before an elementwise apply pass starts; smaller planes run one fused kernel, for which in place is neither
    promised nor tested."""
    lib = _lib.load()
    prec = _prec_of(x)
    B, H, W, Cc = x.shape
    y = _out_or_new(out, tuple(x.shape), x)
    gh, gp = _hostf(gamma)
    bh, bp = _hostf(beta)
    rc = lib.rs_op_groupnorm(x.data_ptr(), y.data_ptr(), gp, bp, film.data_ptr() if film is not None else None, B, H * W, Cc, groups,
                             float(eps), act, prec, _lib.current_stream_ptr())
    _lib.check(rc, "rs_op_groupnorm")
    return y


def window_attention(qkv, table, heads, shift):
    """qkv: [B,H,W,3*heads*32]; table: [225,heads] relative_position_bias_table; returns [B,H,W,heads*32]."""
    lib = _lib.load()
    prec = _prec_of(qkv)
    B, H, W, _ = qkv.shape
    out = torch.empty(B, H, W, heads * 32, device=qkv.device, dtype=qkv.dtype)
    th, tp = _hostf(table)
    rc = lib.rs_op_window_attention(qkv.data_ptr(), out.data_ptr(), tp, B, H, W, heads, shift, prec, _lib.current_stream_ptr())
    _lib.check(rc, "rs_op_window_attention")
    return out


def window_attention_qkv(x, wqkv, bqkv, table, heads, shift, wproj=None, bproj=None, res=None, out=None):
    """x: [B,H,W,E] fp16 normalised tokens; wqkv [3E,E], bqkv [3E]; fused projection + attention (+ output projection wproj
    [E,E], bproj [E] and shortcut `res` when given); returns [B,H,W,E]."""
    lib = _lib.load()
    B, H, W, E = x.shape
    wd = wqkv.to(x.device, torch.float16).contiguous()
    bd = bqkv.to(x.device, torch.float32).contiguous()
    wpd = wproj.to(x.device, torch.float16).contiguous() if wproj is not None else None
    bpd = bproj.to(x.device, torch.float32).contiguous() if bproj is not None else None
    out = _out_or_new(out, (B, H, W, E), x)
    th, tp = _hostf(table)
    rc = lib.rs_op_window_attention_qkv(x.data_ptr(), wd.data_ptr(), bd.data_ptr(), wpd.data_ptr() if wpd is not None else None,
                                        bpd.data_ptr() if bpd is not None else None, res.data_ptr() if res is not None else None, out.data_ptr(),
                                        tp, B, H, W, heads, shift, _lib.current_stream_ptr())
    _lib.check(rc, "rs_op_window_attention_qkv")
    return out


def window_attention_qkv_split(x, wqkv, bqkv, table, heads, shift, wproj=None, bproj=None, res=None, xcoef=None, out=None):
    """split storage: x [B,H,W,E] as int32 carrier ((hi, lo) fp16 pairs); weights any float dtype (packed to (hi, lo) rows here);
    `xcoef` [B,2,E] fp32: GroupNorm affine applied to x on the fly.  Returns [B,H,W,E] split storage."""
    lib = _lib.load()
    B, H, W, E = x.shape
    wd = split_pack_rows(wqkv).to(x.device)
    bd = bqkv.to(x.device, torch.float32).contiguous()
    wpd = split_pack_rows(wproj).to(x.device) if wproj is not None else None
    bpd = bproj.to(x.device, torch.float32).contiguous() if bproj is not None else None
    xc = xcoef.to(x.device, torch.float32).contiguous() if xcoef is not None else None
    out = _out_or_new(out, (B, H, W, E), x)
    th, tp = _hostf(table)
    rc = lib.rs_op_window_attention_qkv_split(x.data_ptr(), wd.data_ptr(), bd.data_ptr(), wpd.data_ptr() if wpd is not None else None,
                                              bpd.data_ptr() if bpd is not None else None, res.data_ptr() if res is not None else None,
                                              out.data_ptr(), tp, xc.data_ptr() if xc is not None else None, B, H, W, heads, shift,
                                              _lib.current_stream_ptr())
    _lib.check(rc, "rs_op_window_attention_qkv_split")
    return out


def ae_flash_attention(q, k, v, bv=None):
    """q, k, v: [nz, T, C] fp16 device tensors -> softmax(q k^T / sqrt(C)) (v + bv), [nz, T, C] fp16 (streaming kernel, ae_attn.hip)"""
    lib = _lib.load()
    nz, T, C = q.shape
    vt = v.transpose(1, 2).contiguous()
    bd = bv.to(q.device, torch.float32).contiguous() if bv is not None else None
    o = torch.empty_like(q)
    rc = lib.rs_op_ae_flash_attention(q.contiguous().data_ptr(), k.contiguous().data_ptr(), vt.data_ptr(), bd.data_ptr() if bd is not None else None,
                                      o.data_ptr(), nz, T, C, _lib.current_stream_ptr())
    _lib.check(rc, "rs_op_ae_flash_attention")
    return o


def ae_flash_attention_split(q, k, v, bv=None):
    """q, k, v: [nz, T, C] fp32 device tensors -> softmax(q k^T / sqrt(C)) (v + bv) computed on (hi, lo) fp16 pairs (three MFMAs per
    product), returned as [nz, T, C] split storage (int32 carrier); streaming kernel ae_attn_split.hip (C = 512, T % 64 == 0)"""
    lib = _lib.load()
    nz, T, C = q.shape
    qs, ks = convert(q.contiguous(), SPLIT), convert(k.contiguous(), SPLIT)
    vts = convert(v.transpose(1, 2).contiguous(), SPLIT)      # [nz, C, T]: rows [T hi | T lo]
    bd = bv.to(q.device, torch.float32).contiguous() if bv is not None else None
    o = torch.empty(nz, T, C, device=q.device, dtype=torch.int32)
    rc = lib.rs_op_ae_flash_attention_split(qs.data_ptr(), ks.data_ptr(), vts.data_ptr(), bd.data_ptr() if bd is not None else None, o.data_ptr(),
                                            nz, T, C, _lib.current_stream_ptr())
    _lib.check(rc, "rs_op_ae_flash_attention_split")
    return o


def split_pack_rows(w):
    """[rows, K] float weights -> the split-storage operand [rows][K hi | K lo] fp16 (hi = fp16(w), lo = fp16((w - hi) 2^11))"""
    w = w.detach().float()
    hi = w.half()
    lo = ((w - hi.float()) * 2048.0).half()
    return torch.cat([hi, lo], dim=1).contiguous()


def swin_mlp(x, w1, b1, w2, b2, res=None):
    """x: [M, E] fp16 (or split storage as int32) device; w1 [HD, E], w2 [E, HD] (any float dtype; rounded to fp16, or to
    (hi, lo) pairs for split storage, like the engine's weights)."""
    lib = _lib.load()
    M, E = x.shape
    HD = w1.shape[0]
    split = x.dtype == torch.int32
    if split:
        w1d, w2d = split_pack_rows(w1).to(x.device), split_pack_rows(w2).to(x.device)
    else:
        w1d, w2d = w1.to(x.device, torch.float16).contiguous(), w2.to(x.device, torch.float16).contiguous()
    b1d, b2d = b1.to(x.device, torch.float32).contiguous(), b2.to(x.device, torch.float32).contiguous()
    y = torch.empty(M, E, device=x.device, dtype=x.dtype)
    fn = lib.rs_op_swin_mlp_split if split else lib.rs_op_swin_mlp
    rc = fn(x.data_ptr(), w1d.data_ptr(), b1d.data_ptr(), w2d.data_ptr(), b2d.data_ptr(), res.data_ptr() if res is not None else None,
            y.data_ptr(), M, E, HD, _lib.current_stream_ptr())
    _lib.check(rc, "swin_mlp")
    return y


def swin_mlp_unembed(x, coef, hw, w1, b1, w2, b2, wu, bu):
    """Last Swin block's MLP half + patch_unembed in one launch (split storage): x [M, E] int32 (hi, lo) pairs = the block's raw input,
    coef [M / hw, 2, E] fp32 = norm2's per-image affine; returns [M, NO] split.  The product matrix [Wu W2 | Wu] and the merged bias are
    formed here in float64 exactly like the engine's packer (csrc/weight_pack.h: rs_unembed_fold_weight)."""
    lib = _lib.load()
    M, E = x.shape
    HD, NO = w1.shape[0], wu.shape[0]
    wcat = torch.cat([wu.double() @ w2.double(), wu.double()], dim=1).float()
    bcat = (wu.double() @ b2.double() + bu.double()).float()
    w1d, wcd = split_pack_rows(w1).to(x.device), split_pack_rows(wcat).to(x.device)
    b1d, bcd = b1.to(x.device, torch.float32).contiguous(), bcat.to(x.device).contiguous()
    cd = coef.to(x.device, torch.float32).contiguous()
    y = torch.empty(M, NO, device=x.device, dtype=x.dtype)
    rc = lib.rs_op_swin_mlp_split_unembed(x.data_ptr(), cd.data_ptr(), w1d.data_ptr(), b1d.data_ptr(), wcd.data_ptr(), bcd.data_ptr(), y.data_ptr(),
                                          M, hw, E, HD, NO, _lib.current_stream_ptr())
    _lib.check(rc, "swin_mlp_unembed")
    return y


def softmax_rows(s, out_prec=F32):
    lib = _lib.load()
    nrows, ncols = s.shape
    out = torch.empty(nrows, ncols, device=s.device, dtype=_dt(out_prec))
    _lib.check(lib.rs_op_softmax_rows(s.data_ptr(), out.data_ptr(), nrows, ncols, out_prec, _lib.current_stream_ptr()), "softmax")
    return out


def vq(z, codebook):
    """z: [N,D] fp32, codebook [NE,D] fp32 (device) -> (zq [N,D], idx [N] int32)."""
    lib = _lib.load()
    N, D = z.shape
    zq = torch.empty_like(z)
    idx = torch.empty(N, device=z.device, dtype=torch.int32)
    _lib.check(lib.rs_op_vq(z.data_ptr(), codebook.data_ptr(), zq.data_ptr(), idx.data_ptr(), N, codebook.shape[0], D,
                            _lib.current_stream_ptr()), "vq")
    return zq, idx


def nchw_to_nhwc(x, prec=F32):
    lib = _lib.load()
    B, Cc, H, W = x.shape
    out = torch.empty(B, H, W, Cc, device=x.device, dtype=_dt(prec))
    _lib.check(lib.rs_op_nchw_to_nhwc(x.data_ptr(), out.data_ptr(), B, Cc, H * W, prec, _lib.current_stream_ptr()), "nchw_to_nhwc")
    return out


def nhwc_to_nchw(x):
    lib = _lib.load()
    B, H, W, Cc = x.shape
    prec = _prec_of(x)
    out = torch.empty(B, Cc, H, W, device=x.device, dtype=torch.float32)
    _lib.check(lib.rs_op_nhwc_to_nchw(x.data_ptr(), out.data_ptr(), B, Cc, H * W, prec, _lib.current_stream_ptr()), "nhwc_to_nchw")
    return out


def bicubic(y, sf):
    """F.interpolate(y, scale_factor=sf, mode='bicubic') on NCHW fp32 (no engine weights needed)."""
    lib = _lib.load()
    B, Cc, H, W = y.shape
    cfg = _lib.Config()
    # a minimal valid config just to own a scratch arena
    cfg.unet.window_size = 8; cfg.unet.num_heads = 1; cfg.unet.swin_embed_dim = 32; cfg.unet.n_levels = 1
    cfg.unet.image_size = 8; cfg.unet.model_channels = 32; cfg.unet.in_channels = 3; cfg.unet.out_channels = 3
    cfg.unet.channel_mult[0] = 1; cfg.unet.num_res_blocks[0] = 1; cfg.unet.swin_depth = 2; cfg.unet.mlp_ratio = 4.0
    cfg.unet.cond_lq = 1; cfg.unet.lq_size = 8
    cfg.has_unet = 1
    cfg.enable_f16 = 1
    e = lib.rs_create(C.byref(cfg))
    if not e:
        raise RuntimeError(_lib.last_error())
    out = torch.empty(B, Cc, H * sf, W * sf, device=y.device, dtype=torch.float32)
    rc = lib.rs_bicubic(e, y.data_ptr(), out.data_ptr(), B, Cc, H, W, sf, _lib.current_stream_ptr())
    torch.cuda.synchronize()
    lib.rs_destroy(e)
    _lib.check(rc, "rs_bicubic")
    return out

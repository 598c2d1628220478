"""ctypes binding of libresshift_hip.so (C ABI: include/resshift_hip.h).

The product path has no CPU fallback: if the HIP library is missing or cannot be loaded this module
raises, loudly.  `import torch` happens first on purpose so that the engine binds to the same
libamdhip64 (soname libamdhip64.so.7) that PyTorch-ROCm already mapped — one HIP runtime per process,
so torch device pointers and streams are valid inside the engine.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from fractions import Fraction

import torch  # noqa: F401  (must precede the CDLL call, see module docstring)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RESSHIFT_HIP_LIB") or os.path.join(HERE, "libresshift_hip.so")   # (override: A/B of two builds on one box)

RS_PREC_F16 = 0
RS_PREC_F32 = 1
RS_PREC_SPLIT = 2
RS_MAX_LEVELS = 8
RS_MAX_STEPS = 64
RS_MAX_ROWS = 64   # most images of one per-image call (include/resshift_hip.h)
RS_COLOR_FIX_WAVELET = 1
RS_COLOR_FIX_ADAIN = 2
COLOR_FIX_MODES = {"wavelet": RS_COLOR_FIX_WAVELET, "adain": RS_COLOR_FIX_ADAIN}


class UNetConfig(C.Structure):
    _fields_ = [
        ("image_size", C.c_int), ("in_channels", C.c_int), ("model_channels", C.c_int), ("out_channels", C.c_int),
        ("n_levels", C.c_int),
        ("channel_mult", C.c_int * RS_MAX_LEVELS),
        ("num_res_blocks", C.c_int * RS_MAX_LEVELS),
        ("n_attn_res", C.c_int),
        ("attention_resolutions", C.c_int * RS_MAX_LEVELS),
        ("swin_depth", C.c_int), ("swin_embed_dim", C.c_int), ("window_size", C.c_int), ("num_heads", C.c_int),
        ("mlp_ratio", C.c_float),
        ("cond_lq", C.c_int), ("cond_mask", C.c_int), ("lq_size", C.c_int),
    ]


class AEConfig(C.Structure):
    _fields_ = [
        ("ch", C.c_int), ("n_levels", C.c_int),
        ("ch_mult", C.c_int * RS_MAX_LEVELS),
        ("num_res_blocks", C.c_int * RS_MAX_LEVELS),
        ("in_channels", C.c_int), ("out_ch", C.c_int), ("z_channels", C.c_int), ("embed_dim", C.c_int),
        ("n_embed", C.c_int), ("resolution", C.c_int),
        ("n_attn_res", C.c_int),
        ("attn_resolutions", C.c_int * RS_MAX_LEVELS),
    ]


class Config(C.Structure):
    _fields_ = [("unet", UNetConfig), ("ae", AEConfig), ("has_unet", C.c_int), ("has_ae", C.c_int), ("enable_f16", C.c_int),
                ("enable_f32", C.c_int), ("enable_split", C.c_int)]


class SampleArgs(C.Structure):
    _fields_ = [
        ("y", C.c_void_p), ("mask", C.c_void_p), ("noise", C.c_void_p), ("out", C.c_void_p), ("z_out", C.c_void_p),
        ("idx_out", C.c_void_p),
        ("B", C.c_int), ("h", C.c_int), ("w", C.c_int), ("sf", C.c_int), ("steps", C.c_int),
        ("inv_std", C.c_float * RS_MAX_STEPS), ("coef1", C.c_float * RS_MAX_STEPS), ("coef2", C.c_float * RS_MAX_STEPS),
        ("sigma", C.c_float * RS_MAX_STEPS), ("tmap", C.c_int * RS_MAX_STEPS),
        ("prior_scale", C.c_float), ("scale_factor", C.c_float),
        ("prec_encode", C.c_int), ("prec_decode", C.c_int), ("prec_unet", C.c_int * RS_MAX_STEPS),
        ("stream", C.c_void_p),
    ]


class StepArgs(C.Structure):
    _fields_ = [
        ("sched", C.POINTER(SampleArgs)), ("x", C.c_void_p), ("pred_xstart", C.c_void_p), ("y", C.c_void_p), ("mask", C.c_void_p),
        ("noise", C.c_void_p), ("t", C.POINTER(C.c_int)), ("B", C.c_int), ("prec", C.c_int), ("stream", C.c_void_p),
    ]


class TileDesc(C.Structure):
    """rs_tile_desc: one tile of the tile pool's gather / scatter launches"""
    _fields_ = [("src", C.c_void_p), ("acc", C.c_void_p), ("count", C.c_void_p),
                ("H", C.c_int), ("W", C.c_int), ("h0", C.c_int), ("w0", C.c_int), ("th", C.c_int), ("tw", C.c_int)]


class NoiseKey(C.Structure):
    """rs_noise_key: `seed` names a request, `stream` a sub-request (tile index inside an image; 0 for a whole image); 16 bytes"""
    _fields_ = [("seed", C.c_uint64), ("stream", C.c_uint32), ("reserved", C.c_uint32)]


def noise_keys(keys):
    """[(seed, stream) | seed | NoiseKey] -> (NoiseKey * n); seeds are taken modulo 2^64, streams must fit 32 bits"""
    arr = (NoiseKey * max(1, len(keys)))()
    for d, k in zip(arr, keys):
        if isinstance(k, NoiseKey):
            d.seed, d.stream, d.reserved = k.seed, k.stream, k.reserved
            continue
        seed, stream = (k if isinstance(k, (tuple, list)) else (k, 0))
        if not 0 <= int(stream) < 2 ** 32:
            raise ValueError(f"noise key stream {stream} does not fit 32 bits")
        d.seed, d.stream, d.reserved = int(seed) % 2 ** 64, int(stream), 0
    return arr


_P, _I, _F, _LL, _SZ = C.c_void_p, C.c_int, C.c_float, C.c_longlong, C.c_size_t

# name -> (restype, argtypes); every symbol declared in include/resshift_hip.h is listed here.
SIGNATURES = {
    "rs_create": (_P, [C.POINTER(Config)]),
    "rs_destroy": (None, [_P]),
    "rs_last_error": (C.c_char_p, []),
    "rs_load_tensor": (_I, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), _I]),
    "rs_weight_bytes": (_SZ, [_P]),
    "rs_bind_weight_blob": (_I, [_P, _P, _SZ]),
    "rs_pack_weights": (_I, [_P]),
    "rs_bcast_weights": (_I, [_P, _P, _I, _P]),
    "rs_weights_ready": (_I, [_P]),
    "rs_unet_forward": (_I, [_P, _P, C.POINTER(C.c_int), _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "rs_vq_encode": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "rs_vq_decode": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "rs_bicubic": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "rs_sample": (_I, [_P, C.POINTER(SampleArgs)]),
    "rs_sample_begin": (_I, [_P, C.POINTER(SampleArgs), _P]),
    "rs_sample_step": (_I, [_P, C.POINTER(StepArgs)]),
    "rs_sample_end": (_I, [_P, C.POINTER(SampleArgs), _P]),
    "rs_film_prewarm": (_I, [_P, C.POINTER(C.c_int), _I, _P]),
    "rs_axpbypcz": (_I, [_P, _P, _P, _P, _F, _F, _F, _LL, _P]),
    "rs_axpbypcz_rows": (_I, [_P, _P, _P, _P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), _LL, _I, _P]),
    "rs_noise_fill": (_I, [C.POINTER(NoiseKey), C.POINTER(C.c_int), _P, _LL, _I, _P]),
    "rs_sample_seeded": (_I, [_P, C.POINTER(SampleArgs), C.POINTER(NoiseKey)]),
    "rs_sample_begin_seeded": (_I, [_P, C.POINTER(SampleArgs), _P, C.POINTER(NoiseKey)]),
    "rs_sample_step_seeded": (_I, [_P, C.POINTER(StepArgs), C.POINTER(NoiseKey)]),
    "rs_tile_accumulate": (_I, [_P, _P, _P] + [_I] * 8 + [_P]),
    "rs_tile_finalize": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "rs_window_copy": (_I, [_P, _P, _LL, _I, _I, _I, _I, _I, _I, _F, _P]),
    "rs_tile_gather": (_I, [C.POINTER(TileDesc), _I, _I, _P, _P, _I, _I, _P]),
    "rs_tile_scatter": (_I, [C.POINTER(TileDesc), _I, _I, _I, _P, _I, _I, _P]),
    "rs_tile_accumulate_weighted": (_I, [_P, _P, _P] + [_I] * 10 + [_P]),
    "rs_tile_scatter_weighted": (_I, [C.POINTER(TileDesc), _I, _I, _I, _P, _I, _I, _I, _I, _P]),
    "rs_color_fix_work_bytes": (_SZ, [_I] * 6),
    "rs_color_fix": (_I, [_P, _P, _P] + [_I] * 6 + [_P, _SZ, _P]),
    "rs_resize": (_I, [_P, _P] + [_I] * 6 + [C.c_double, C.c_double, _I, _P]),
    "rs_metrics_work_bytes": (_SZ, [_I] * 6),
    "rs_metrics": (_I, [_P, _P] + [_I] * 8 + [_P, _P, _P, _SZ, _P]),
    "rs_rgb_to_y_u8": (_I, [_P, _P, _SZ, _P]),
    "rs_filter2d": (_I, [_P, _P, _P] + [_I] * 7 + [_P]),
    "rs_interp": (_I, [_P, _P] + [_I] * 6 + [C.c_double, C.c_double, _I, _I, _P]),
    "rs_jpeg": (_I, [_P, _P, C.POINTER(C.c_float)] + [_I] * 4 + [_P]),
    "rs_add_noise": (_I, [_P, _P, C.POINTER(NoiseKey), C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_int)] + [_I] * 5 + [_P]),
    "rs_unit_to_u8": (_I, [_P, _P] + [_I] * 4 + [_P]),
    "rs_jpeg_codec": (_I, [_P, _P, C.POINTER(C.c_int)] + [_I] * 4 + [_P]),
    "rs_blur_resize": (_I, [_P, _P, _P] + [_I] * 9 + [_P]),
    "rs_u8_to_input": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "rs_output_to_u8": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "rs_arena_bytes": (_SZ, [_P]),
    "rs_last_launch_count": (_LL, [_P]),
    "rs_profile_enable": (_I, [_P, _I]),
    "rs_profile_get": (_I, [_P, C.POINTER(C.c_double)]),
    "rs_profile_families": (_I, [_P, C.POINTER(C.c_double), _I]),
    "rs_profile_shapes": (_I, [_P, C.c_char_p, _I]),
    "rs_debug_enable": (_I, [_P, _I]),
    "rs_debug_count": (_I, [_P]),
    "rs_debug_info": (_I, [_P, _I, C.c_char_p, _I, C.POINTER(C.c_int)]),
    "rs_debug_fetch": (_I, [_P, _I, _P, _P]),
    "rs_debug_fetch_rows": (_I, [_P, _I, _I, _I, _P, _P]),
    "rs_op_conv2d": (_I, [_P, _P, _P, _P, _P, _P] + [_I] * 18 + [_P]),
    "rs_op_conv2d_ex": (_I, [_P, _P, _P, _P, _P, _P] + [_I] * 22 + [C.POINTER(C.c_int), _P]),
    "rs_op_conv_plan": (_I, [_I] * 23 + [C.POINTER(C.c_int)]),
    "rs_op_conv2d_bench": (_I, [_P, _P, _P, _P, _P] + [_I] * 16 + [C.POINTER(C.c_float), _P]),
    "rs_op_conv3x3_halo_stats_px": (_I, [_I, _I, _I, _I, _I, _I]),
    "rs_op_conv3x3_halo": (_I, [_P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "rs_op_conv3x3_wino": (_I, [_P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _I, C.POINTER(C.c_float), _P]),
    "rs_op_gemm_nt": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _F, _I, _I, _P]),
    "rs_op_groupnorm": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _I, _I, _P]),
    "rs_op_window_attention": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "rs_op_window_attention_qkv": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "rs_op_window_attention_qkv_split": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "rs_op_swin_mlp": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "rs_op_ae_flash_attention": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "rs_op_ae_flash_attention_split": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "rs_op_swin_mlp_split": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "rs_op_swin_mlp_split_unembed": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "rs_op_softmax_rows": (_I, [_P, _P, _LL, _I, _I, _P]),
    "rs_op_vq": (_I, [_P, _P, _P, _P, _LL, _I, _I, _P]),
    "rs_op_nchw_to_nhwc": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "rs_op_nhwc_to_nchw": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "rs_op_convert": (_I, [_P, _I, _P, _I, _I, _LL, _P]),
}

_lib = None


def load() -> C.CDLL:
    """Load the HIP engine; raises RuntimeError (never falls back) when it is not available."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m resshift_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback for the ResShift hot path."
        )
    try:
        lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    except OSError as e:  # pragma: no cover
        raise RuntimeError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error() -> str:
    return load().rs_last_error().decode()


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        raise RuntimeError(f"resshift_hip {what} failed (rc={rc}): {last_error()}")


def current_stream_ptr() -> int:
    """hipStream_t of torch's current stream (0 = null stream when torch has no GPU)."""
    if torch.cuda.is_available():
        return int(torch.cuda.current_stream().cuda_stream)
    return 0


def window_copy(x, h0=0, w0=0, ho=None, wo=None, scale=1.0, out=None):
    """fp32 device tensor [..., H, W] -> [..., ho, wo] window starting at (h0, w0), reflected past the bottom / right edge and
    multiplied by `scale` (rs_window_copy: reflect padding, tile crops and the latent scaling of the host mirror).  The result is
    always float32 (the engine's user-facing tensors are fp32 like the reference's inference path; F.pad / slicing in the
    reference keep the input dtype, which is float32 there too)."""
    import torch

    if not x.is_cuda:
        raise RuntimeError("window_copy needs a device tensor: the host mirror does not fall back to CPU arithmetic")
    x = x.to(torch.float32).contiguous()
    H, W = x.shape[-2:]
    ho = H if ho is None else ho
    wo = W if wo is None else wo
    planes = x.numel() // (H * W)
    want = (*x.shape[:-2], ho, wo)
    if out is None:
        out = torch.empty(*want, device=x.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or tuple(out.shape) != want or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"window_copy: `out` must be a contiguous float32 tensor of shape {want} on {x.device} "
                         f"(got {out.dtype}, {tuple(out.shape)}, contiguous={out.is_contiguous()}, {out.device})")
    check(load().rs_window_copy(x.data_ptr(), out.data_ptr(), planes, H, W, h0, w0, ho, wo, float(scale), current_stream_ptr()), "rs_window_copy")
    return out


def _tile_descs(rows):
    arr = (TileDesc * len(rows))()
    for d, r in zip(arr, rows):
        d.src, d.acc, d.count, d.H, d.W, d.h0, d.w0, d.th, d.tw = r
    return arr


def tile_gather(tiles, out_lq, out_mask=None):
    """rs_tile_gather: `tiles` = [(src [C_src,H,W] fp32 device tensor, h0, w0, th, tw)], at most RS_MAX_ROWS, possibly of different images
    (one C_src); writes their windows, reflect-padded on the bottom / right to out_lq's [n,3,Hp,Wp] (and out_mask's [n,1,Hp,Wp] from
    plane 3 when C_src is 4).  One launch, no allocation: the outputs are the caller's (contiguous fp32, e.g. rows of a dense pool)."""
    n = len(tiles)
    Hp, Wp = out_lq.shape[-2:]
    for t in (out_lq, out_mask):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape[0] == n):
            raise ValueError(f"tile_gather: outputs must be contiguous float32 device tensors with {n} rows")
    for src, *_ in tiles:
        if not (src.is_cuda and src.dtype == torch.float32 and src.is_contiguous() and src.dim() == 3 and src.shape[0] == tiles[0][0].shape[0]):
            raise ValueError("tile_gather: every source must be a contiguous float32 device tensor [C_src,H,W] with the same C_src")
    descs = _tile_descs([(src.data_ptr(), None, None, src.shape[1], src.shape[2], h0, w0, th, tw) for src, h0, w0, th, tw in tiles])
    check(load().rs_tile_gather(descs, n, int(tiles[0][0].shape[0]) if n else 0, out_lq.data_ptr(), out_mask.data_ptr() if out_mask is not None else None,
                                Hp, Wp, current_stream_ptr()), "rs_tile_gather")


def tile_scatter(tiles, batch, sf, ramp=None):
    """rs_tile_scatter: `tiles` = [(acc [C,H*sf,W*sf], count [H*sf,W*sf], H, W, h0, w0, th, tw)] for the rows of `batch` [n,C,Hp_out,Wp_out]:
    adds each row's top-left (th*sf) x (tw*sf) crop into its canvas window and 1 into the count there - one launch, the bits of
    rs_tile_accumulate called tile by tile in index order (tiles of one launch may overlap).
    `ramp` = (Rh, Rw) in HR pixels: rs_tile_scatter_weighted instead - feathered blending, the crop and the count weighted down towards
    the tile's edges (include/resshift_hip.h), the bits of tile_accumulate_weighted tile by tile."""
    n = len(tiles)
    if not (batch.is_cuda and batch.dtype == torch.float32 and batch.is_contiguous() and batch.dim() == 4 and batch.shape[0] == n):
        raise ValueError(f"tile_scatter: the tiles must be one contiguous float32 device tensor [{n},C,Hp,Wp]")
    Cc = int(batch.shape[1])
    for acc, cnt, H, W, *_ in tiles:
        if not (acc.is_cuda and acc.dtype == cnt.dtype == torch.float32 and acc.is_contiguous() and cnt.is_contiguous()
                and tuple(acc.shape) == (Cc, H * sf, W * sf) and tuple(cnt.shape) == (H * sf, W * sf)):
            raise ValueError(f"tile_scatter: a canvas must be contiguous float32 [{Cc},H*sf,W*sf] with its count plane [H*sf,W*sf]")
    descs = _tile_descs([(None, acc.data_ptr(), cnt.data_ptr(), H, W, h0, w0, th, tw) for acc, cnt, H, W, h0, w0, th, tw in tiles])
    if ramp is None:
        check(load().rs_tile_scatter(descs, n, Cc, int(sf), batch.data_ptr(), int(batch.shape[2]), int(batch.shape[3]), current_stream_ptr()), "rs_tile_scatter")
    else:
        check(load().rs_tile_scatter_weighted(descs, n, Cc, int(sf), batch.data_ptr(), int(batch.shape[2]), int(batch.shape[3]), int(ramp[0]),
                                              int(ramp[1]), current_stream_ptr()), "rs_tile_scatter_weighted")


def tile_accumulate_weighted(acc, count, tile, h0, w0, ramp):
    """rs_tile_accumulate_weighted: canvas acc [B,C,H,W] and its count plane [H,W] (HR pixels) += the feather-weighted `tile` [B,C,th,tw]
    at (h0, w0); `ramp` = (Rh, Rw) in HR pixels.  Contiguous fp32 device tensors."""
    B, Cc, H, W = acc.shape
    th, tw = tile.shape[2:]
    for t, shape in ((acc, (B, Cc, H, W)), (count, (H, W)), (tile, (B, Cc, th, tw))):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError("tile_accumulate_weighted: acc [B,C,H,W], count [H,W] and tile [B,C,th,tw] must be contiguous float32 device tensors")
    check(load().rs_tile_accumulate_weighted(acc.data_ptr(), count.data_ptr(), tile.data_ptr(), B, Cc, H, W, int(h0), int(w0), th, tw,
                                             int(ramp[0]), int(ramp[1]), current_stream_ptr()), "rs_tile_accumulate_weighted")


def tile_finalize(acc, count):
    """rs_tile_finalize on one image's canvas [C,H,W] and its count plane [H,W] (contiguous fp32 device tensors): acc /= count in place"""
    Cc, H, W = acc.shape
    check(load().rs_tile_finalize(acc.data_ptr(), count.data_ptr(), 1, Cc, H, W, current_stream_ptr()), "rs_tile_finalize")
    return acc


def color_fix(sr, lq, mode):
    """rs_color_fix: the sample sr [B,C,H*sf,W*sf] corrected against its input lq [B,C,H,W] (contiguous fp32 device tensors in [-1,1]; sf
    = the integer ratio of their sizes), `mode` "wavelet" | "adain" (include/resshift_hip.h).  Returns a new tensor; the scratch of the
    adain statistics is a torch tensor of rs_color_fix_work_bytes bytes that lives until the call's stream work is done."""
    if mode not in COLOR_FIX_MODES:
        raise ValueError(f"unknown colour fix {mode!r} (one of {sorted(COLOR_FIX_MODES)})")
    for t in (sr, lq):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 4):
            raise ValueError("color_fix: sr [B,C,H*sf,W*sf] and lq [B,C,H,W] must be contiguous float32 device tensors")
    B, Cc, H, W = lq.shape
    sf = sr.shape[2] // H
    if sf < 1 or tuple(sr.shape) != (B, Cc, H * sf, W * sf):
        raise ValueError(f"color_fix: sr {tuple(sr.shape)} is no integer multiple of lq {tuple(lq.shape)}")
    lib = load()
    m = COLOR_FIX_MODES[mode]
    need = int(lib.rs_color_fix_work_bytes(B, Cc, H, W, sf, m))
    work = torch.empty(need, device=sr.device, dtype=torch.uint8) if need else None
    out = torch.empty_like(sr)
    check(lib.rs_color_fix(sr.data_ptr(), lq.data_ptr(), out.data_ptr(), B, Cc, H, W, sf, m, work.data_ptr() if need else None, need,
                           current_stream_ptr()), "rs_color_fix")
    return out


RESIZE_SCALES = (0.125, 8.0)   # rs_resize holds at most ceil(4 * 8) + 2 = 34 taps per axis


def resize_len(n, scale) -> int:
    """ceil(n * scale), exactly: the scale is taken as the nearest fraction of denominator <= 4096 (0.3 * 40 is 12)"""
    return math.ceil(int(n) * Fraction(scale).limit_denominator(4096))


def resize(x, scale=None, size=None, clamp=False):
    """rs_resize: x [B,C,H,W] (a contiguous fp32 device tensor) resized with MATLAB's antialiased bicubic imresize (include/resshift_hip.h).
    Exactly one of `scale` - a number for both axes; the output is ceil(H * scale) x ceil(W * scale), as imresize_np has it - and `size`
    = (Ho, Wo), which gives the per-axis scales Ho / H and Wo / W.  `clamp`: clamp the result to [-1, 1].  Returns a new tensor."""
    if (scale is None) == (size is None):
        raise ValueError("resize: give exactly one of scale and size")
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4):
        raise ValueError("resize: x [B,C,H,W] must be a contiguous float32 device tensor")
    B, Cc, H, W = x.shape
    if scale is not None:
        if isinstance(scale, bool) or not isinstance(scale, (int, float, Fraction)) or not scale > 0:
            raise ValueError(f"resize: scale must be a positive number, not {scale!r}")
        Ho, Wo = resize_len(H, scale), resize_len(W, scale)
        sh = sw = float(scale)
    else:
        if not (isinstance(size, (tuple, list)) and len(size) == 2 and all(isinstance(v, int) and not isinstance(v, bool) and v > 0 for v in size)):
            raise ValueError(f"resize: size must be two positive integers (Ho, Wo), not {size!r}")
        Ho, Wo = size
        sh, sw = Ho / H, Wo / W
    if not all(RESIZE_SCALES[0] <= s <= RESIZE_SCALES[1] for s in (sh, sw)):
        raise ValueError(f"resize: the scales ({sh:.6g}, {sw:.6g}) of {H} x {W} -> {Ho} x {Wo} must lie in [1/8, 8]")
    out = torch.empty((B, Cc, Ho, Wo), device=x.device, dtype=torch.float32)
    check(load().rs_resize(x.data_ptr(), out.data_ptr(), B, Cc, H, W, Ho, Wo, sh, sw, 1 if clamp else 0, current_stream_ptr()), "rs_resize")
    return out


# ---- degradation operators (include/resshift_hip.h "degradation") -------------------------------------------------------
FILTER_KMAX = 21
INTERP_MODES = {"area": 0, "bilinear": 1, "bicubic": 2}


def _image_batch(x, who):
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4):
        raise ValueError(f"{who}: x [B,C,H,W] must be a contiguous float32 device tensor")
    return tuple(int(v) for v in x.shape)


def filter2d(x, kernels, clamp=False):
    """rs_filter2d: x [B,C,H,W] cross-correlated (the kernel is not flipped) with `kernels` [Bk,k,k] behind torch's `reflect` padding - the
    reference's filter2D.  Bk is 1 (one kernel for the batch) or B (one per image, for all its channels); k is odd, at most 21, and k // 2
    is below min(H, W).  `clamp` clamps the result to [0, 1].  Contiguous fp32 device tensors; returns a new tensor."""
    B, Cc, H, W = _image_batch(x, "filter2d")
    if not (isinstance(kernels, torch.Tensor) and kernels.is_cuda and kernels.dtype == torch.float32 and kernels.is_contiguous() and kernels.dim() == 3
            and kernels.shape[1] == kernels.shape[2] and kernels.device == x.device):
        raise ValueError("filter2d: kernels [Bk,k,k] must be a contiguous float32 tensor on x's device")
    Bk, k = int(kernels.shape[0]), int(kernels.shape[1])
    if k % 2 == 0 or k > FILTER_KMAX:
        raise ValueError(f"filter2d: k must be odd and at most {FILTER_KMAX}, not {k}")
    if k // 2 >= min(H, W):
        raise ValueError(f"filter2d: k // 2 = {k // 2} must be below min(H, W) = {min(H, W)} (one reflection per border)")
    if Bk not in (1, B):
        raise ValueError(f"filter2d: {Bk} kernels for {B} images (1 or B)")
    out = torch.empty_like(x)
    check(load().rs_filter2d(x.data_ptr(), kernels.data_ptr(), out.data_ptr(), B, Cc, H, W, k, Bk, 1 if clamp else 0, current_stream_ptr()), "rs_filter2d")
    return out


def interp_size(n, scale_factor) -> int:
    """floor(n * scale_factor) in float64: F.interpolate's output length for a scale factor"""
    return int(math.floor(float(n) * float(scale_factor)))


def interpolate(x, scale_factor=None, size=None, mode="bilinear", clamp=False):
    """rs_interp: F.interpolate(x, scale_factor= | size=, mode="area" | "bilinear" | "bicubic", align_corners=False) without antialiasing on
    a contiguous fp32 device tensor [B,C,H,W] - the resize of the degradation recipe (`resize` is MATLAB's antialiased one).  Exactly one
    of `scale_factor` (a number for both axes: output floor(H * s), coordinates step by 1 / s) and `size` = (Ho, Wo) (coordinates step by H
    / Ho).  The scales must lie in [1/8, 8].  `clamp` clamps the result to [0, 1].  Returns a new tensor."""
    B, Cc, H, W = _image_batch(x, "interpolate")
    if mode not in INTERP_MODES:
        raise ValueError(f"interpolate: unknown mode {mode!r} (one of {sorted(INTERP_MODES)})")
    if (scale_factor is None) == (size is None):
        raise ValueError("interpolate: give exactly one of scale_factor and size")
    if scale_factor is not None:
        if isinstance(scale_factor, bool) or not isinstance(scale_factor, (int, float)) or not scale_factor > 0:
            raise ValueError(f"interpolate: scale_factor must be a positive number, not {scale_factor!r}")
        s = float(scale_factor)
        Ho, Wo, sh, sw = interp_size(H, s), interp_size(W, s), s, s
        inside = RESIZE_SCALES[0] <= s <= RESIZE_SCALES[1] and Ho >= 1 and Wo >= 1
    else:
        if not (isinstance(size, (tuple, list)) and len(size) == 2 and all(isinstance(v, int) and not isinstance(v, bool) and v > 0 for v in size)):
            raise ValueError(f"interpolate: size must be two positive integers (Ho, Wo), not {size!r}")
        Ho, Wo = size
        sh = sw = 0.0
        inside = all(RESIZE_SCALES[0] <= v <= RESIZE_SCALES[1] for v in (Ho / H, Wo / W))
    if not inside:
        raise ValueError(f"interpolate: the scales of {H} x {W} -> {Ho} x {Wo} must lie in [1/8, 8]")
    out = torch.empty((B, Cc, Ho, Wo), device=x.device, dtype=torch.float32)
    check(load().rs_interp(x.data_ptr(), out.data_ptr(), B, Cc, H, W, Ho, Wo, sh, sw, INTERP_MODES[mode], 1 if clamp else 0, current_stream_ptr()),
          "rs_interp")
    return out


def _per_image(values, B, who, what):
    vals = [values] * B if isinstance(values, (int, float)) and not isinstance(values, bool) else list(values)
    if len(vals) != B:
        raise ValueError(f"{who}: {B} images but {len(vals)} {what}")
    return vals


def jpeg(x, quality):
    """rs_jpeg: the reference's DiffJPEG(differentiable=False) on x [B,3,H,W] (a contiguous fp32 device tensor in [0,1] - the caller clamps),
    `quality` one number per image (or one for all) in (0, 100) exclusive.  Batches above RS_MAX_ROWS go in chunks (the qualities travel by
    value).  Returns a new tensor."""
    B, Cc, H, W = _image_batch(x, "jpeg")
    if Cc != 3:
        raise ValueError(f"jpeg: C must be 3 (RGB), not {Cc}")
    q = [float(v) for v in _per_image(quality, B, "jpeg", "qualities")]
    if not all(0.0 < v < 100.0 for v in q):
        raise ValueError(f"jpeg: every quality must lie in (0, 100), not {q}")
    out = torch.empty_like(x)
    lib = load()
    for b0 in range(0, B, RS_MAX_ROWS):
        n = min(RS_MAX_ROWS, B - b0)
        check(lib.rs_jpeg(x[b0:].data_ptr(), out[b0:].data_ptr(), (C.c_float * n)(*q[b0:b0 + n]), n, 3, H, W, current_stream_ptr()), "rs_jpeg")
    return out


def add_noise(x, keys, sigma, gray=False, draw=0, clamp=True):
    """rs_add_noise: x [B,C,H,W] + (sigma[b] / 255) n, clamped to [0, 1] unless clamp=False.  n = the normals `noise_fill` gives for
    (keys[b], draw[b]) and the shape (C, H, W); an image whose `gray` flag is set takes those for (1, H, W) in every channel.  `sigma`, `gray`
    and `draw` are one value per image or one for all.  Returns a new tensor."""
    B, Cc, H, W = _image_batch(x, "add_noise")
    if len(keys) != B:
        raise ValueError(f"add_noise: {B} images but {len(keys)} keys")
    sg = [float(v) for v in _per_image(sigma, B, "add_noise", "sigmas")]
    gr = [int(bool(v)) for v in ([gray] * B if isinstance(gray, (bool, int)) else _per_image(gray, B, "add_noise", "gray flags"))]
    dr = [int(v) for v in _per_image(draw, B, "add_noise", "draw indices")]
    if not all(math.isfinite(v) and v >= 0 for v in sg):
        raise ValueError(f"add_noise: every sigma must be finite and not negative, not {sg}")
    if any(v < 0 for v in dr):
        raise ValueError(f"add_noise: negative draw index in {dr}")
    out = torch.empty_like(x)
    lib = load()
    for b0 in range(0, B, RS_MAX_ROWS):
        n = min(RS_MAX_ROWS, B - b0)
        s = slice(b0, b0 + n)
        check(lib.rs_add_noise(x[b0:].data_ptr(), out[b0:].data_ptr(), noise_keys(list(keys[s])), (C.c_int * n)(*dr[s]), (C.c_float * n)(*sg[s]),
                               (C.c_int * n)(*gr[s]), n, Cc, H, W, 1 if clamp else 0, current_stream_ptr()), "rs_add_noise")
    return out


def unit_to_u8(x):
    """rs_unit_to_u8: fp32 [B,C,H,W] in [0,1] (a contiguous device tensor) -> uint8 [B,H,W,C] = clamp(rint(x * 255), 0, 255), ties to even"""
    B, Cc, H, W = _image_batch(x, "unit_to_u8")
    out = torch.empty((B, H, W, Cc), device=x.device, dtype=torch.uint8)
    check(load().rs_unit_to_u8(x.data_ptr(), out.data_ptr(), B, Cc, H, W, current_stream_ptr()), "rs_unit_to_u8")
    return out


# ---- face degradation operators (include/resshift_hip.h "face degradation") ----------------------------------------------
BLUR_RESIZE_KMAX = 41
BLUR_RESIZE_SCALES = (1.0 / 64, 64.0)
JPEG_CODEC_MIN = 8   # rs_jpeg_codec: the least height and width


def jpeg_codec(x, quality):
    """rs_jpeg_codec: libjpeg's baseline JPEG round trip at 4:2:0 (cv2's imencode + imdecode, PIL's save(quality=q, subsampling=2) + open) on
    x [B,3,H,W] in RGB order, a contiguous fp32 device tensor that is clipped to [0, 1] and rounded to 8 bits; H, W >= 8; `quality` one
    integer per image (or one for all) in 1 .. 100.  Batches above RS_MAX_ROWS go in chunks.  Returns a new tensor on the 1/255 grid."""
    B, Cc, H, W = _image_batch(x, "jpeg_codec")
    if Cc != 3:
        raise ValueError(f"jpeg_codec: C must be 3 (RGB), not {Cc}")
    if H < JPEG_CODEC_MIN or W < JPEG_CODEC_MIN:
        raise ValueError(f"jpeg_codec: H and W must be at least {JPEG_CODEC_MIN}, not {H} x {W}")
    q = [quality] * B if isinstance(quality, bool) else _per_image(quality, B, "jpeg_codec", "qualities")
    if not all(isinstance(v, int) and not isinstance(v, bool) and 1 <= v <= 100 for v in q):
        raise ValueError(f"jpeg_codec: every quality must be an integer in 1 .. 100, not {q}")
    out = torch.empty_like(x)
    lib = load()
    for b0 in range(0, B, RS_MAX_ROWS):
        n = min(RS_MAX_ROWS, B - b0)
        check(lib.rs_jpeg_codec(x[b0:].data_ptr(), out[b0:].data_ptr(), (C.c_int * n)(*q[b0:b0 + n]), n, 3, H, W, current_stream_ptr()), "rs_jpeg_codec")
    return out


def blur_resize(x, kernels, size, clamp=False):
    """rs_blur_resize: bilinear(filter2d(x, kernels), size=(Ho, Wo)) in one launch, the filter evaluated only where the resize reads it.  x
    [B,C,H,W] and kernels [Bk,k,k] as `filter2d` takes them, with k odd and at most 41; `kernels=None`: the bilinear resize alone.  The
    scales Ho / H and Wo / W must lie in [1/64, 64].  `clamp` clamps the result to [0, 1].  Returns a new tensor."""
    B, Cc, H, W = _image_batch(x, "blur_resize")
    if not (isinstance(size, (tuple, list)) and len(size) == 2 and all(isinstance(v, int) and not isinstance(v, bool) and v > 0 for v in size)):
        raise ValueError(f"blur_resize: size must be two positive integers (Ho, Wo), not {size!r}")
    Ho, Wo = size
    Bk = k = 0
    if kernels is not None:
        if not (isinstance(kernels, torch.Tensor) and kernels.is_cuda and kernels.dtype == torch.float32 and kernels.is_contiguous() and kernels.dim() == 3
                and kernels.shape[1] == kernels.shape[2] and kernels.device == x.device):
            raise ValueError("blur_resize: kernels [Bk,k,k] must be a contiguous float32 tensor on x's device (or None)")
        Bk, k = int(kernels.shape[0]), int(kernels.shape[1])
        if k % 2 == 0 or k > BLUR_RESIZE_KMAX:
            raise ValueError(f"blur_resize: k must be odd and at most {BLUR_RESIZE_KMAX}, not {k}")
        if k // 2 >= min(H, W):
            raise ValueError(f"blur_resize: k // 2 = {k // 2} must be below min(H, W) = {min(H, W)} (one reflection per border)")
        if Bk not in (1, B):
            raise ValueError(f"blur_resize: {Bk} kernels for {B} images (1 or B)")
    if not all(BLUR_RESIZE_SCALES[0] <= v <= BLUR_RESIZE_SCALES[1] for v in (Ho / H, Wo / W)):
        raise ValueError(f"blur_resize: the scales of {H} x {W} -> {Ho} x {Wo} must lie in [1/64, 64]")
    out = torch.empty((B, Cc, Ho, Wo), device=x.device, dtype=torch.float32)
    check(load().rs_blur_resize(x.data_ptr(), kernels.data_ptr() if kernels is not None else None, out.data_ptr(), B, Cc, H, W, Ho, Wo, k, Bk,
                                1 if clamp else 0, current_stream_ptr()), "rs_blur_resize")
    return out


METRICS_TAPS = 11   # the SSIM window: the cropped image must be at least 11 x 11


def _metrics_input(t, who):
    """(is_float, B, C, H, W) of one input of `metrics`: uint8 [B,H,W,C] or float32 [B,C,H,W]"""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 4 and t.is_contiguous() and t.dtype in (torch.uint8, torch.float32)):
        raise ValueError(f"metrics: {who} must be a contiguous device tensor, uint8 [B,H,W,C] or float32 [B,C,H,W] in [-1,1]")
    if t.dtype == torch.uint8:
        B, H, W, Cc = t.shape
        return 0, B, Cc, H, W
    B, Cc, H, W = t.shape
    return 1, B, Cc, H, W


def metrics(a, b, border=0, ycbcr=True):
    """rs_metrics: PSNR / SSIM of the image batch `a` against `b` on uint8 pixels (include/resshift_hip.h "image metrics").  Each input is a
    contiguous device tensor, uint8 [B,H,W,C] or float32 [B,C,H,W] in [-1,1] (quantised as rs_output_to_u8 does); C is 1 or 3; `ycbcr`
    (C == 3) scores MATLAB's Y channel; `border` pixels are cropped from every side and at least 11 x 11 must remain.  Returns
    {"psnr": float64 [B], "ssim": float64 [B], "sse": int64 [B]} on the device: sse and ssim come from the kernels, psnr =
    20 log10(255 / sqrt(sse / n)) from float64 torch ops on sse (inf at sse == 0) - nothing waits for the stream."""
    fa, B, Cc, H, W = _metrics_input(a, "a")
    fb, *shape_b = _metrics_input(b, "b")
    if tuple(shape_b) != (B, Cc, H, W):
        raise ValueError(f"metrics: a is {B} images of {H} x {W} x {Cc}, b is {shape_b[0]} images of {shape_b[2]} x {shape_b[3]} x {shape_b[1]}")
    if Cc not in (1, 3):
        raise ValueError(f"metrics: C must be 1 or 3, not {Cc}")
    if isinstance(border, bool) or not isinstance(border, int) or border < 0:
        raise ValueError(f"metrics: border must be a non-negative integer, not {border!r}")
    ycbcr = bool(ycbcr)
    if ycbcr and Cc != 3:
        raise ValueError(f"metrics: ycbcr=True needs C == 3, not {Cc}")
    Hc, Wc = H - 2 * border, W - 2 * border
    if Hc < METRICS_TAPS or Wc < METRICS_TAPS:
        raise ValueError(f"metrics: the cropped image is {Hc} x {Wc} ({H} x {W}, border {border}): the 11 x 11 window needs at least 11 x 11")
    if a.device != b.device:
        raise ValueError(f"metrics: a is on {a.device}, b on {b.device}")
    lib = load()
    need = int(lib.rs_metrics_work_bytes(B, Cc, H, W, border, int(ycbcr)))
    work = torch.empty(need // 8, device=a.device, dtype=torch.int64)
    sse = torch.empty(B, device=a.device, dtype=torch.int64)
    ssim = torch.empty(B, device=a.device, dtype=torch.float64)
    check(lib.rs_metrics(a.data_ptr(), b.data_ptr(), fa, fb, B, Cc, H, W, border, int(ycbcr), sse.data_ptr(), ssim.data_ptr(), work.data_ptr(),
                         need, current_stream_ptr()), "rs_metrics")
    n = (1 if ycbcr else Cc) * Hc * Wc
    psnr = 20.0 * torch.log10(255.0 / torch.sqrt(sse.to(torch.float64) / n))
    return {"psnr": psnr, "ssim": ssim, "sse": sse}


def rgb_to_y(rgb):
    """rs_rgb_to_y_u8: uint8 [...,3] (a contiguous device tensor) -> uint8 [...]: MATLAB's rounded luma, 16 + round((65481 r + 128553 g +
    24966 b) / 255000) in exact integer arithmetic, ties to even"""
    if not (isinstance(rgb, torch.Tensor) and rgb.is_cuda and rgb.dtype == torch.uint8 and rgb.is_contiguous() and rgb.dim() >= 1
            and rgb.shape[-1] == 3 and rgb.numel() > 0):
        raise ValueError("rgb_to_y: rgb must be a non-empty contiguous uint8 device tensor [...,3]")
    out = torch.empty(rgb.shape[:-1], device=rgb.device, dtype=torch.uint8)
    check(load().rs_rgb_to_y_u8(rgb.data_ptr(), out.data_ptr(), rgb.numel() // 3, current_stream_ptr()), "rs_rgb_to_y_u8")
    return out

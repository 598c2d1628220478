"""ctypes binding of libresshift_hip.so (C ABI: include/resshift_hip.h).

The product path has no CPU fallback: if the HIP library is missing or cannot be loaded this module
raises, loudly.  `import torch` happens first on purpose so that the engine binds to the same
libamdhip64 (soname libamdhip64.so.7) that PyTorch-ROCm already mapped — one HIP runtime per process,
so torch device pointers and streams are valid inside the engine.
"""
from __future__ import annotations

import ctypes as C
import os

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
    "rs_jpeg_encode_bound": (_SZ, [_I, _I]),
    "rs_jpeg_encode_workspace": (_SZ, [_I, _I, _I]),
    "rs_jpeg_encode": (_I, [_P, _P, _P, C.POINTER(C.c_int), _P] + [_I] * 4 + [_SZ, _P]),
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


def __getattr__(name):
    """the image operators live in imageops.py; `_lib.filter2d` and the like still find them (resolved on use: imageops imports this module)"""
    from . import imageops

    if name in imageops.__all__:
        return getattr(imageops, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")

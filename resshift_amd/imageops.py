"""The image operators around the sampler (include/resshift_hip.h "colour correction" .. "JPEG files"): the argument
checks and the ctypes call of each as a module function on contiguous device tensors, and `ImageOps`, the same on a device for callers
that hand over any float tensor - `Engine` inherits it, `degrade.Degrader` builds one when it has no engine.  `_lib.<name>` still finds
every public name of this module."""
from __future__ import annotations

import ctypes as C
import math
from fractions import Fraction

import torch

from ._lib import COLOR_FIX_MODES, RS_MAX_ROWS, check, current_stream_ptr, load, noise_keys

__all__ = ["ImageOps", "color_fix", "RESIZE_SCALES", "resize_len", "resize", "FILTER_KMAX", "INTERP_MODES", "filter2d", "interp_size", "interpolate",
           "jpeg", "add_noise", "unit_to_u8", "BLUR_RESIZE_KMAX", "BLUR_RESIZE_SCALES", "JPEG_CODEC_MIN", "jpeg_codec", "blur_resize",
           "JPEG_ENCODE_MAX", "jpeg_encode_bound", "jpeg_encode",
           "METRICS_TAPS", "metrics", "rgb_to_y"]


def _size_arg(who, size):
    """(Ho, Wo) of a `size` argument"""
    if not (isinstance(size, (tuple, list)) and len(size) == 2 and all(isinstance(v, int) and not isinstance(v, bool) and v > 0 for v in size)):
        raise ValueError(f"{who}: size must be two positive integers (Ho, Wo), not {size!r}")
    return size


def _kernels_arg(who, x, kernels, kmax, optional=False):
    """(Bk, k) of the filter kernels [Bk,k,k] for the image batch x; (0, 0) for kernels=None where the operator takes that"""
    if optional and kernels is None:
        return 0, 0
    B, _, H, W = x.shape
    if not (isinstance(kernels, torch.Tensor) and kernels.is_cuda and kernels.dtype == torch.float32 and kernels.is_contiguous() and kernels.dim() == 3
            and kernels.shape[1] == kernels.shape[2] and kernels.device == x.device):
        raise ValueError(f"{who}: kernels [Bk,k,k] must be a contiguous float32 tensor on x's device" + (" (or None)" if optional else ""))
    Bk, k = int(kernels.shape[0]), int(kernels.shape[1])
    if k % 2 == 0 or k > kmax:
        raise ValueError(f"{who}: k must be odd and at most {kmax}, not {k}")
    if k // 2 >= min(H, W):
        raise ValueError(f"{who}: k // 2 = {k // 2} must be below min(H, W) = {min(H, W)} (one reflection per border)")
    if Bk not in (1, B):
        raise ValueError(f"{who}: {Bk} kernels for {B} images (1 or B)")
    return Bk, k


def _row_chunks(B):
    """the slices of at most RS_MAX_ROWS images of a batch of B: the per-image arguments travel by value"""
    return [slice(b0, min(b0 + RS_MAX_ROWS, B)) for b0 in range(0, B, RS_MAX_ROWS)]


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
        Ho, Wo = _size_arg("resize", size)
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
    Bk, k = _kernels_arg("filter2d", x, kernels, FILTER_KMAX)
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
        Ho, Wo = _size_arg("interpolate", size)
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


def _qualities(who, quality, B):
    """one integer quality 1 .. 100 per image, from one for all or a sequence of B"""
    q = [quality] * B if isinstance(quality, bool) else _per_image(quality, B, who, "qualities")
    if not all(isinstance(v, int) and not isinstance(v, bool) and 1 <= v <= 100 for v in q):
        raise ValueError(f"{who}: every quality must be an integer in 1 .. 100, not {q}")
    return q


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
    for s in _row_chunks(B):
        n = s.stop - s.start
        check(lib.rs_jpeg(x[s].data_ptr(), out[s].data_ptr(), (C.c_float * n)(*q[s]), n, 3, H, W, current_stream_ptr()), "rs_jpeg")
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
    for s in _row_chunks(B):
        n = s.stop - s.start
        check(lib.rs_add_noise(x[s].data_ptr(), out[s].data_ptr(), noise_keys(list(keys[s])), (C.c_int * n)(*dr[s]), (C.c_float * n)(*sg[s]),
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
    q = _qualities("jpeg_codec", quality, B)
    out = torch.empty_like(x)
    lib = load()
    for s in _row_chunks(B):
        n = s.stop - s.start
        check(lib.rs_jpeg_codec(x[s].data_ptr(), out[s].data_ptr(), (C.c_int * n)(*q[s]), n, 3, H, W, current_stream_ptr()), "rs_jpeg_codec")
    return out


def blur_resize(x, kernels, size, clamp=False):
    """rs_blur_resize: bilinear(filter2d(x, kernels), size=(Ho, Wo)) in one launch, the filter evaluated only where the resize reads it.  x
    [B,C,H,W] and kernels [Bk,k,k] as `filter2d` takes them, with k odd and at most 41; `kernels=None`: the bilinear resize alone.  The
    scales Ho / H and Wo / W must lie in [1/64, 64].  `clamp` clamps the result to [0, 1].  Returns a new tensor."""
    B, Cc, H, W = _image_batch(x, "blur_resize")
    Ho, Wo = _size_arg("blur_resize", size)
    Bk, k = _kernels_arg("blur_resize", x, kernels, BLUR_RESIZE_KMAX, optional=True)
    if not all(BLUR_RESIZE_SCALES[0] <= v <= BLUR_RESIZE_SCALES[1] for v in (Ho / H, Wo / W)):
        raise ValueError(f"blur_resize: the scales of {H} x {W} -> {Ho} x {Wo} must lie in [1/64, 64]")
    out = torch.empty((B, Cc, Ho, Wo), device=x.device, dtype=torch.float32)
    check(load().rs_blur_resize(x.data_ptr(), kernels.data_ptr() if kernels is not None else None, out.data_ptr(), B, Cc, H, W, Ho, Wo, k, Bk,
                                1 if clamp else 0, current_stream_ptr()), "rs_blur_resize")
    return out


# ---- JPEG files (include/resshift_hip.h "JPEG files") --------------------------------------------------------------------
JPEG_ENCODE_MAX = 65535   # rs_jpeg_encode: the largest height and width (the SOF0 fields)


def jpeg_encode_bound(H, W) -> int:
    """rs_jpeg_encode_bound: the bytes a JPEG file of an H x W image can reach - the header, every block at its longest code with every
    byte of the scan stuffed, EOI"""
    return int(load().rs_jpeg_encode_bound(int(H), int(W)))


def jpeg_encode(x, quality):
    """rs_jpeg_encode: the images x -> their baseline JPEG files, one `bytes` per image, each byte for byte what
    PIL.Image.save(format="JPEG", quality=q, subsampling=2) writes.  x is a contiguous device tensor, uint8 [B,H,W,3] in RGB order (what
    `output_to_u8` / `unit_to_u8` return) or float32 [B,3,H,W] in [0,1], which `unit_to_u8` rounds first - rint(clip(x, 0, 1) * 255), the
    input step of `jpeg_codec`; 8 <= H, W <= 65535; `quality` one integer per image (or one for all) in 1 .. 100.  Batches above
    RS_MAX_ROWS go in chunks.  The files are coded on the device; per chunk one device-to-host copy of the lengths and one of the used
    bytes of the rows - never the rows' bound."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.is_contiguous() and x.dim() == 4 and x.dtype in (torch.uint8, torch.float32)):
        raise ValueError("jpeg_encode: x must be a contiguous device tensor, uint8 [B,H,W,3] or float32 [B,3,H,W] in [0,1]")
    B = int(x.shape[0])
    Cc, H, W = (int(x.shape[3]), int(x.shape[1]), int(x.shape[2])) if x.dtype == torch.uint8 else (int(v) for v in x.shape[1:])
    if Cc != 3:
        raise ValueError(f"jpeg_encode: C must be 3 (RGB), not {Cc}")
    if B < 1:
        raise ValueError("jpeg_encode: an empty batch")
    if not (JPEG_CODEC_MIN <= H <= JPEG_ENCODE_MAX and JPEG_CODEC_MIN <= W <= JPEG_ENCODE_MAX):
        raise ValueError(f"jpeg_encode: H and W must lie in {JPEG_CODEC_MIN} .. {JPEG_ENCODE_MAX}, not {H} x {W}")
    q = _qualities("jpeg_encode", quality, B)
    lib = load()
    u8 = x if x.dtype == torch.uint8 else unit_to_u8(x)
    pitch = (int(lib.rs_jpeg_encode_bound(H, W)) + 255) // 256 * 256
    files = []
    for s in _row_chunks(B):
        n = s.stop - s.start
        need = int(lib.rs_jpeg_encode_workspace(n, H, W))
        if need == 0:
            raise ValueError(f"jpeg_encode: {H} x {W} is too large (rs_jpeg_encode takes about 55 megapixels)")
        out = torch.empty((n, pitch), device=x.device, dtype=torch.uint8)
        work = torch.empty(need, device=x.device, dtype=torch.uint8)
        nbytes = torch.empty(n, device=x.device, dtype=torch.int32)
        check(lib.rs_jpeg_encode(u8[s].data_ptr(), out.data_ptr(), nbytes.data_ptr(), (C.c_int * n)(*q[s]), work.data_ptr(), n, 3, H, W, pitch,
                                 current_stream_ptr()), "rs_jpeg_encode")
        lens = nbytes.cpu().tolist()
        host = out[:, :max(lens)].cpu().numpy()       # (the columns any file of the chunk uses)
        files += [host[i, :lens[i]].tobytes() for i in range(n)]
    return files


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


class ImageOps:
    """The image operators on `device` for any float tensor: detached, converted to contiguous fp32 and run under torch.cuda.device(device)."""

    def __init__(self, device=None):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())

    @staticmethod
    def _f32c(t: torch.Tensor) -> torch.Tensor:
        return t.detach().to(torch.float32).contiguous()

    def color_fix(self, sr, lq, mode="wavelet"):
        """The sample sr [B,C,H*sf,W*sf] corrected against its input lq [B,C,H,W], both in [-1,1]: "wavelet" keeps sr's detail and takes
        the low frequencies of the bicubic up-sampled lq, "adain" takes lq's per-channel mean and deviation (rs_color_fix).
        Returns a new tensor; whole images only - tiles are corrected after they are blended."""
        with torch.cuda.device(self.device):
            return color_fix(self._f32c(sr), self._f32c(lq), mode)

    def resize(self, x, scale=None, size=None, clamp=False):
        """x [B,C,H,W] resized with MATLAB's antialiased bicubic imresize (rs_resize): `scale` for both axes (output
        ceil(H * scale) x ceil(W * scale)) or `size` = (Ho, Wo); `clamp` clamps the result to [-1, 1].  Returns a new fp32 tensor; whole
        images only - tiles are resized after they are blended."""
        with torch.cuda.device(self.device):
            return resize(self._f32c(x), scale=scale, size=size, clamp=clamp)

    # the degradation operators (resshift_amd/degrade.py runs them in the recipe's order): images in [0, 1], new tensors
    def filter2d(self, x, kernels, clamp=False):
        """The reference's filter2D: x [B,C,H,W] cross-correlated with `kernels` [1 | B,k,k] behind `reflect` padding (rs_filter2d)."""
        with torch.cuda.device(self.device):
            return filter2d(self._f32c(x), self._f32c(kernels), clamp=clamp)

    def interpolate(self, x, scale_factor=None, size=None, mode="bilinear", clamp=False):
        """F.interpolate(x, scale_factor= | size=, mode="area" | "bilinear" | "bicubic") without antialiasing (rs_interp); `resize` is
        MATLAB's antialiased resize."""
        with torch.cuda.device(self.device):
            return interpolate(self._f32c(x), scale_factor=scale_factor, size=size, mode=mode, clamp=clamp)

    def jpeg(self, x, quality):
        """The reference's DiffJPEG(differentiable=False) on x [B,3,H,W] in [0,1], one quality in (0, 100) per image (rs_jpeg)."""
        with torch.cuda.device(self.device):
            return jpeg(self._f32c(x), quality)

    def add_noise(self, x, keys, sigma, gray=False, draw=0, clamp=True):
        """x + (sigma / 255) n with n = noise_fill(keys, draw, (C | 1, H, W)) generated in registers, clamped to [0, 1] (rs_add_noise)."""
        with torch.cuda.device(self.device):
            return add_noise(self._f32c(x), keys, sigma, gray=gray, draw=draw, clamp=clamp)

    def unit_to_u8(self, x):
        """fp32 [B,C,H,W] in [0,1] -> uint8 [B,H,W,C], clamp(rint(x * 255), 0, 255) (rs_unit_to_u8)."""
        with torch.cuda.device(self.device):
            return unit_to_u8(self._f32c(x))

    # the face recipe's operators
    def jpeg_codec(self, x, quality):
        """libjpeg's baseline JPEG round trip at 4:2:0 on x [B,3,H,W] (RGB, clipped to [0,1]), one integer quality 1 .. 100 per image
        (rs_jpeg_codec): cv2's imencode + imdecode, byte for byte."""
        with torch.cuda.device(self.device):
            return jpeg_codec(self._f32c(x), quality)

    def blur_resize(self, x, kernels, size, clamp=False):
        """bilinear(filter2d(x, kernels), size) in one launch with kernels of up to 41 taps; kernels=None: the resize alone (rs_blur_resize)."""
        with torch.cuda.device(self.device):
            return blur_resize(self._f32c(x), None if kernels is None else self._f32c(kernels), size, clamp=clamp)

    # JPEG files
    def jpeg_encode(self, x, quality):
        """x - uint8 [B,H,W,3] RGB, or a float tensor [B,3,H,W] in [0,1] - as baseline JPEG files coded on the device, one `bytes` per image
        and one integer quality 1 .. 100 per image: byte for byte PIL's save(format="JPEG", quality=q, subsampling=2) (rs_jpeg_encode)."""
        with torch.cuda.device(self.device):
            return jpeg_encode(x.detach().contiguous() if x.dtype == torch.uint8 else self._f32c(x), quality)

    def metrics(self, sr, gt, border=0, ycbcr=True):
        """PSNR / SSIM of the batch `sr` against the ground truth `gt` on uint8 pixels, as the reference's calculate_psnr / calculate_ssim
        score them (rs_metrics).  Each is uint8 [B,H,W,C] or a float tensor [B,C,H,W] in [-1,1], which is quantised exactly
        as `output_to_u8` does; C is 1 or 3; `ycbcr` scores MATLAB's Y channel (C == 3); `border` pixels are cropped from every side.
        Returns {"psnr": float64 [B], "ssim": float64 [B], "sse": int64 [B]} on the device."""
        prep = lambda t: t.contiguous() if t.dtype == torch.uint8 else self._f32c(t)
        with torch.cuda.device(self.device):
            return metrics(prep(sr), prep(gt), border=border, ycbcr=ycbcr)

    def rgb_to_y(self, u8):
        """uint8 [...,3] device tensor -> uint8 [...]: MATLAB's rounded Y channel in exact integer arithmetic (rs_rgb_to_y_u8)"""
        with torch.cuda.device(self.device):
            return rgb_to_y(u8.contiguous())

"""libjpeg's baseline JPEG round trip (4:2:0, "islow" DCT, fancy up-sampling, default tables) restated in numpy integer arithmetic:
what `PIL save(quality=q, subsampling=2)` + `open` and cv2's imencode + imdecode compute, and the definition of rs_jpeg_codec
(include/resshift_hip.h).  The entropy stage is lossless and is left out.  Everything is int64 here; no intermediate
reaches 2^31, so the device's int32 arithmetic is the same function.  `>>` is an arithmetic shift.  `mut` names one of MUTATIONS: the
plausible mistakes that tests/test_face_degrade_cpu.py shows the recorded cases to catch."""
import numpy as np

LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], np.int64).reshape(8, 8)      # Annex K, natural order: [vertical frequency][horizontal]
CHROMA = np.full((8, 8), 99, np.int64)
CHROMA[:4, :4] = [[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]]


def FIX16(c):
    return int(c * 65536 + .5)


def FIX13(c):
    return int(c * 8192 + .5)


def DESCALE(x, n):
    return (x + (1 << (n - 1))) >> n


C0_298, C0_390, C0_541, C0_765, C0_899, C1_175, C1_501, C1_847, C1_961, C2_053, C2_562, C3_072 = (FIX13(c) for c in (
    0.298631336, 0.390180644, 0.541196100, 0.765366865, 0.899976223, 1.175875602, 1.501321110, 1.847759065, 1.961570560, 2.053119869,
    2.562915447, 3.072711026))


MUTATIONS = ("constant_bias", "cbcr_32768", "fullres_bottom", "truncating_quantiser", "swapped_upsample_bias", "no_end_columns",
             "upsample_reads_padding", "transposed_luma")


def quant_table(base, quality):
    """jpeg_set_quality(quality, force_baseline=TRUE) of the Annex K table `base`"""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quality {quality} is outside 1 .. 100")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((base * s + 50) // 100, 1, 255)


def _odd(t0, t1, t2, t3):
    """the odd part both transforms share, on (t0, t1, t2, t3) = forward (t4, t5, t6, t7) / inverse (i7, i5, i3, i1): returns the four sums"""
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * C1_175
    t0, t1, t2, t3 = t0 * C0_298, t1 * C2_053, t2 * C3_072, t3 * C1_501
    z1, z2, z3, z4 = z1 * -C0_899, z2 * -C2_562, z3 * -C1_961 + z5, z4 * -C0_390 + z5
    return t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4


def _fdct8(d, rows):
    """one pass of jfdctint.c over the last axis; rows=True is the first (row) pass"""
    d = [d[..., i] for i in range(8)]
    t0, t1, t2, t3 = d[0] + d[7], d[1] + d[6], d[2] + d[5], d[3] + d[4]
    t7, t6, t5, t4 = d[0] - d[7], d[1] - d[6], d[2] - d[5], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if rows else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if rows else DESCALE(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if rows else DESCALE(t10 - t11, 2)
    z1 = (t12 + t13) * C0_541
    o[2] = DESCALE(z1 + t13 * C0_765, n)
    o[6] = DESCALE(z1 - t12 * C1_847, n)
    s7, s5, s3, s1 = _odd(t4, t5, t6, t7)
    o[7], o[5], o[3], o[1] = DESCALE(s7, n), DESCALE(s5, n), DESCALE(s3, n), DESCALE(s1, n)
    return np.stack(o, axis=-1)


def _idct8(i, cols):
    """one pass of jidctint.c over the last axis; cols=True is the first (column) pass"""
    i = [i[..., k] for k in range(8)]
    z1 = (i[2] + i[6]) * C0_541
    t2, t3 = z1 - i[6] * C1_847, z1 + i[2] * C0_765
    t0, t1 = (i[0] + i[4]) << 13, (i[0] - i[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = _odd(i[7], i[5], i[3], i[1])
    n = 11 if cols else 18
    out = [t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3]
    return np.stack([DESCALE(v, n) for v in out], axis=-1)


def _blocks(plane):
    """[8 m, 8 n] -> [m, n, 8, 8]"""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def _unblocks(b):
    m, n = b.shape[:2]
    return b.transpose(0, 2, 1, 3).reshape(m * 8, n * 8)


def code_plane(plane, table, mut=None):
    """[8 m, 8 n] samples 0 .. 255 -> the decoded samples: - 128, forward DCT (rows, then columns), quantise, dequantise, inverse DCT
    (columns, then rows), + 128, clamp"""
    b = _blocks(plane.astype(np.int64) - 128)
    c = _fdct8(b, True)                                             # along each row
    c = _fdct8(c.swapaxes(-1, -2), False).swapaxes(-1, -2)          # along each column: c[u, v], u the vertical frequency
    d = 8 * table
    q = np.sign(c) * ((np.abs(c) + (0 if mut == "truncating_quantiser" else d >> 1)) // d)
    w = q * table
    w = _idct8(w.swapaxes(-1, -2), True).swapaxes(-1, -2)           # along each column
    w = _idct8(w, False)                                            # along each row
    return np.clip(_unblocks(w) + 128, 0, 255)


def _pad_edge(p, rows, cols):
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def forward_planes(rgb, mut=None):
    """uint8 [H,W,3] RGB -> (Y [Hm,Wm], Cb, Cr [Hm/2,Wm/2]) padded to the MCU multiple as libjpeg pads them"""
    H, W = rgb.shape[:2]
    Hm, Wm = -(-H // 16) * 16, -(-W // 16) * 16
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (FIX16(.299) * r + FIX16(.587) * g + FIX16(.114) * b + 32768) >> 16
    half = 32768 if mut == "cbcr_32768" else 32767
    cb = (-FIX16(.16874) * r - FIX16(.33126) * g + FIX16(.5) * b + (128 << 16) + half) >> 16
    cr = (FIX16(.5) * r - FIX16(.41869) * g - FIX16(.08131) * b + (128 << 16) + half) >> 16
    He = Hm if mut == "fullres_bottom" else H + (H & 1)             # the bottom: full resolution up to an even row count only
    bias = np.tile(np.array([2, 2] if mut == "constant_bias" else [1, 2], np.int64), Wm // 4)   # 1 on even output columns, 2 on odd ones, every row alike
    planes = [_pad_edge(y, Hm, Wm)]
    for c in (cb, cr):
        c = _pad_edge(c, He, Wm)
        ds = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias[None, :]) >> 2
        planes.append(_pad_edge(ds, Hm // 2, Wm // 2))              # the down-sampled rows are what is replicated
    return planes


def fancy_upsample(c, H, W, mut=None):
    """h2v2 "fancy" (triangle) up-sampling of the real ceil(H / 2) x ceil(W / 2) chroma samples `c` -> [2 ceil(H/2), 2 ceil(W/2)]"""
    c = (c if mut == "upsample_reads_padding" else c[:(H + 1) // 2, :(W + 1) // 2]).astype(np.int64)
    up = np.concatenate([c[:1], c[:-1]], axis=0)                    # the row above (the first row stands in for itself)
    dn = np.concatenate([c[1:], c[-1:]], axis=0)
    s = np.stack([3 * c + up, 3 * c + dn], axis=1).reshape(2 * c.shape[0], c.shape[1])
    left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    if mut == "no_end_columns":                                     # (the mirrored neighbour instead of the sample itself)
        left, right = np.concatenate([s[:, 1:2], s[:, :-1]], axis=1), np.concatenate([s[:, 1:], s[:, -2:-1]], axis=1)
    be, bo = (7, 8) if mut == "swapped_upsample_bias" else (8, 7)
    even, odd = (3 * s + left + be) >> 4, (3 * s + right + bo) >> 4   # (at the ends 3 s + s = 4 s)
    return np.stack([even, odd], axis=2).reshape(s.shape[0], 2 * s.shape[1])


def roundtrip(rgb, quality, mut=None):
    """uint8 [H,W,3] RGB -> uint8 [H,W,3]: encode at `quality` (1 .. 100, 4:2:0) and decode"""
    rgb = np.asarray(rgb)
    H, W = rgb.shape[:2]
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or H < 1 or W < 1:
        raise ValueError("roundtrip: uint8 [H,W,3]")
    assert mut is None or mut in MUTATIONS, mut
    ty, tc = quant_table(LUMA.T if mut == "transposed_luma" else LUMA, quality), quant_table(CHROMA, quality)
    y, cb, cr = forward_planes(rgb, mut)
    y = code_plane(y, ty, mut)[:H, :W]
    cb = fancy_upsample(code_plane(cb, tc, mut), H, W, mut)[:H, :W] - 128
    cr = fancy_upsample(code_plane(cr, tc, mut), H, W, mut)[:H, :W] - 128
    r = y + ((FIX16(1.402) * cr + 32768) >> 16)
    b = y + ((FIX16(1.772) * cb + 32768) >> 16)
    g = y + ((-FIX16(.34414) * cb - FIX16(.71414) * cr + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def to_u8(x):
    """rs_jpeg_codec's input step on fp32 [3,H,W] -> uint8 [H,W,3]: rint(clip(x, 0, 1) * 255) in fp32, ties to even"""
    x = np.asarray(x, np.float32)
    v = np.minimum(np.maximum(x, np.float32(0)), np.float32(1)) * np.float32(255)
    return np.rint(v).astype(np.uint8).transpose(1, 2, 0)


def codec(x, quality):
    """fp32 [B,3,H,W], qualities [B] -> fp32 [B,3,H,W]: rs_jpeg_codec as a function"""
    out = [roundtrip(to_u8(xi), q).transpose(2, 0, 1).astype(np.float32) / np.float32(255) for xi, q in zip(x, quality)]
    return np.stack(out).astype(np.float32)


def pillow_roundtrip(rgb, quality):
    import io

    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", quality=int(quality), subsampling=2)
    buf.seek(0)
    return np.asarray(Image.open(buf).convert("RGB"))


# ---------------------------------------------------------------------------------------------------------------- recorded cases
# what scripts/make_golden_jpeg.py runs through Pillow and tests/golden/libjpeg_roundtrip.npz holds.  The sizes cover the codec's edge
# rules: one MCU and less (8 x 8, 16 x 16, 9 x 8); odd and padded (17 x 33); H = 8 (mod 16) for the bottom rule and W = 8 for the Y block
# that no image data fills (24 x 72, 40 x 56); 31 x 50, 64 x 48, 48 x 64; and 80 x 144, more than one 64 x 128 tile of the kernel on both axes.
SIZES = [(8, 8), (16, 16), (9, 8), (17, 33), (24, 72), (40, 56), (31, 50), (64, 48), (48, 64), (80, 144)]
QUALITIES = [1, 30, 49, 50, 69, 95, 100]
CONTENTS = ["random", "smooth", "binary", "constant", "float"]


def content(kind, H, W, seed):
    """fp32 [3,H,W]: uniform random bytes / 255, a smooth field, random 0 / 255 (which saturates the IDCT into the clamp), a constant, and
    values off the 1/255 grid with exact .5 ties of the fp32 product and values outside [0, 1]"""
    rng = np.random.default_rng(seed)
    if kind == "random":
        return (rng.integers(0, 256, (3, H, W)).astype(np.float32) / np.float32(255)).astype(np.float32)
    if kind == "smooth":
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        ph = rng.uniform(0, 6.28, 3)
        return np.stack([0.5 + 0.45 * np.sin(xx / 5.0 + yy / 7.0 + ph[0]), (xx + 2 * yy) / (W + 2 * H), 0.5 + 0.5 * np.cos(xx * yy / 97.0 + ph[2])]).astype(np.float32)
    if kind == "binary":
        return rng.integers(0, 2, (3, H, W)).astype(np.float32)
    if kind == "constant":
        return np.broadcast_to(np.array([0.8, 0.3, 0.55], np.float32)[:, None, None], (3, H, W)).copy()
    if kind == "float":
        x = rng.uniform(-0.2, 1.2, (3, H, W)).astype(np.float32)
        ties = ((rng.integers(0, 255, (3, H, W)).astype(np.float32) + np.float32(0.5)) / np.float32(255)).astype(np.float32)
        return np.where(rng.random((3, H, W)) < 0.3, ties, x).astype(np.float32)
    raise KeyError(kind)


def case_quality(si, ci):
    """the quality of the recorded case (size si, content ci): every quality meets every content over the sizes"""
    return QUALITIES[(si + 3 * ci) % len(QUALITIES)]


def cases():
    """[(key, (H, W), content kind, seed, quality)]"""
    return [(f"{H}x{W}_{kind}", (H, W), kind, 1000 + 10 * si + ci, case_quality(si, ci))
            for si, (H, W) in enumerate(SIZES) for ci, kind in enumerate(CONTENTS)]

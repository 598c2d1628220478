"""Float64 restatement of the degradation operators (include/resshift_hip.h "degradation"), written from their definitions:
the filter, the JPEG stage, the noise addition, the uint8 rounding and the execution of a plan stage.  Resizes call F.interpolate on
float64 CPU tensors - that IS the definition; `bicubic` restates it once more so that its constant can be mutated.  Every function takes
and returns float64 numpy arrays [B,C,H,W].  The keyword arguments beyond the definition's are the mutations tests/test_degrade_cpu.py
shows the GPU bounds to catch."""
import hashlib

import numpy as np
import torch
import torch.nn.functional as F

# the JPEG standard's Annex K tables, row-major as printed there; the reference indexes their transposes
Y_TABLE = np.array([[16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56],
                    [14, 17, 22, 29, 51, 87, 80, 62], [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92],
                    [49, 64, 78, 87, 103, 121, 120, 101], [72, 92, 95, 98, 112, 100, 103, 99]], dtype=np.float64).T
C_TABLE = np.full((8, 8), 99.0)
C_TABLE[:4, :4] = np.array([[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]], dtype=np.float64).T
# the matrices as float32 roundings (they are float32 parameters in the reference), used in float64
FWD = np.array([[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]], dtype=np.float32).astype(np.float64)
INV = np.array([[1.0, 0.0, 1.402], [1.0, -0.344136, -0.714136], [1.0, 1.772, 0.0]], dtype=np.float32).astype(np.float64)
_ALPHA = np.array([1.0 / np.sqrt(2.0)] + [1.0] * 7)
ALPHA2 = np.outer(_ALPHA, _ALPHA).astype(np.float32).astype(np.float64)
SCALE = (np.outer(_ALPHA, _ALPHA) * 0.25).astype(np.float32).astype(np.float64)
COS = np.array([[np.cos((2 * y + 1) * v * np.pi / 16) for v in range(8)] for y in range(8)]).astype(np.float32).astype(np.float64)   # [y][v]


def inputs(shape, seed):
    """uniform in [0, 1), float32, from a fixed numpy seed"""
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


def digest(a) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------- recorded cases
# what scripts/make_golden_degrade.py runs through the reference and tests/golden/reference_degrade.npz holds (inputs: B = 2, C = 3,
# `inputs((2, 3, H, W), seed)`; kernels: resshift_amd.degrade.KernelSpec parameters, one per batch or one per image)
#   (key, (H, W), seed, [KernelSpec arguments])
FILTER_CASES = [
    ("k3_shared", (12, 14), 11, [dict(kind="iso", size=3, pad_to=3, sig_x=0.6, sig_y=0.6)]),
    ("k7_per_image", (16, 20), 12, [dict(kind="aniso", size=5, pad_to=7, sig_x=0.5, sig_y=1.4, theta=0.7),
                                    dict(kind="sinc", size=7, pad_to=7, cutoff=1.5)]),
    ("k13_per_image", (24, 30), 13, [dict(kind="sinc", size=11, pad_to=13, cutoff=1.2),
                                     dict(kind="generalized_aniso", size=13, pad_to=13, sig_x=2.0, sig_y=0.8, theta=-1.1, beta=1.3)]),
    ("k21_shared", (26, 40), 14, [dict(kind="sinc", size=21, pad_to=21, cutoff=0.9)]),
    ("k21_per_image", (26, 40), 15, [dict(kind="plateau_iso", size=21, pad_to=21, sig_x=3.0, sig_y=3.0, beta=1.1),
                                     dict(kind="aniso", size=21, pad_to=21, sig_x=4.0, sig_y=2.0, theta=2.5)]),
]
#   (key, (H, W), qualities, seed): constructed_jpeg_case
JPEG_CASES = [("q30_70", (32, 48), (30.0, 70.0), 21), ("q95_50", (32, 48), (95.0, 50.0), 22), ("q10_99", (32, 48), (10.0, 99.0), 23)]
#   (key, builder of the reference, arguments)
BUILDER_CASES = [
    ("gauss_iso", "bivariate_Gaussian", dict(kernel_size=13, sig_x=0.7, sig_y=0.7, theta=0.0, isotropic=True)),
    ("gauss_aniso", "bivariate_Gaussian", dict(kernel_size=7, sig_x=0.4, sig_y=1.8, theta=-2.2, isotropic=False)),
    ("general_iso", "bivariate_generalized_Gaussian", dict(kernel_size=9, sig_x=1.5, sig_y=1.5, theta=0.0, beta=0.6, isotropic=True)),
    ("general_aniso", "bivariate_generalized_Gaussian", dict(kernel_size=21, sig_x=3.0, sig_y=1.0, theta=1.0, beta=1.4, isotropic=False)),
    ("plateau_iso", "bivariate_plateau", dict(kernel_size=5, sig_x=0.9, sig_y=0.9, theta=0.0, beta=1.15, isotropic=True)),
    ("plateau_aniso", "bivariate_plateau", dict(kernel_size=11, sig_x=2.5, sig_y=0.7, theta=0.3, beta=1.05, isotropic=False)),
    ("sinc_small", "circular_lowpass_kernel", dict(cutoff=2.7, kernel_size=5, pad_to=7)),
    ("sinc_large", "circular_lowpass_kernel", dict(cutoff=0.7, kernel_size=21, pad_to=0)),
]


# The distance of the reference's OWN all-fp32 outputs from this float64 restatement, per operator, as tests/test_degrade_cpu.py
# measures it (it asserts that its measurement lies in (REF_ERR / 2, REF_ERR]); the bounds of tests/test_degrade_gpu.py are five times
# these - a kernel in fp32 has no reason to be farther from float64 than the reference is, and gets the factor for another summation order:
#   filter2D 9.2e-7 (k = 21, FILTER_CASES);  F.interpolate fp32 against float64 2.4e-6 (bicubic at a fractional scale, INTERP_CASES);
#   DiffJPEG on the constructed inputs 4.8e-7 (JPEG_CASES).
REF_ERR = {"filter": 1.0e-6, "interp": 3.0e-6, "jpeg": 5.0e-7}
TOL = {k: 5.0 * v for k, v in REF_ERR.items()}
TIE_DELTA = 1e-3   # natural JPEG inputs: an MCU beyond the bound must hold a pre-round coefficient this close to a half-integer

# the shapes of the GPU tests (B = 2, C = 3)
#   (key, (H, W), seed, [KernelSpec arguments]): smaller than a tile with a reflection 10 deep; across a tile edge on both axes.  Every
#   kernel of the recipe equals its own flip (k[u, v] = k[-u, -v]); kind "raw" is a seeded random kernel with sum 1, which does not
GPU_FILTER_CASES = [
    ("small_k21_shared", (11, 13), 16, [dict(kind="raw", size=21, seed=41)]),
    ("small_k21_per_image", (11, 13), 17, [dict(kind="sinc", size=21, pad_to=21, cutoff=1.1),
                                           dict(kind="aniso", size=19, pad_to=21, sig_x=3.0, sig_y=5.0, theta=-0.9)]),
    ("tiles_k3_shared", (24, 72), 18, [dict(kind="raw", size=3, seed=42)]),
    ("tiles_k3_per_image", (24, 72), 19, [dict(kind="iso", size=3, pad_to=3, sig_x=0.7, sig_y=0.7),
                                          dict(kind="aniso", size=3, pad_to=3, sig_x=0.9, sig_y=0.3, theta=2.0)]),
    ("tiles_k13_shared", (24, 72), 20, [dict(kind="sinc", size=11, pad_to=13, cutoff=1.7)]),
    ("tiles_k13_per_image", (24, 72), 24, [dict(kind="raw", size=13, seed=43),
                                           dict(kind="plateau_aniso", size=9, pad_to=13, sig_x=1.5, sig_y=0.6, theta=-0.5, beta=1.1)]),
]
#   from (24, 40): two scale factors and two sizes, every mode
INTERP_SHAPE, INTERP_SEED = (24, 40), 31
INTERP_CASES = [(mode, kind, v) for mode in ("area", "bilinear", "bicubic")
                for kind, v in (("scale_factor", 0.73), ("scale_factor", 1.37), ("size", (6, 10)), ("size", (31, 47)))]


def natural_images(root, crop=None):
    """8 images of tests/golden/val_sr_lq.npz as float32 [8,3,64,64] in [0,1]; crop = (h, w): their top-left corner"""
    x = (np.load(f"{root}/tests/golden/val_sr_lq.npz")["lq"][:8].astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2)
    return np.ascontiguousarray(x if crop is None else x[:, :, :crop[0], :crop[1]])


TIE_QUALITY = 75.0


def tie_image(B=2, H=16, W=32):
    """An input whose chroma DC coefficient is EXACTLY 22.5 at quality 75 (factor 1/2), in fp32 and in float64 alike, every step exact: R =
    G = 0 and B = 0.1875, so 255 B = 47.8125, Cb - 128 = 23.90625 on every sample, the block sum is 1530 and 0.125 * 1530 / (17 * 0.5) =
    22.5.  Ties go to even - 22; rounding half away from zero gives 23 and moves the blue channel by 0.007."""
    x = np.zeros((B, 3, H, W), np.float32)
    x[:, 2] = 0.1875
    return x


def filter_case(case):
    """(x float32 [2,3,H,W], kernels float32 [Bk,k,k]) of a FILTER_CASES entry"""
    from resshift_amd.degrade import KernelSpec

    _, shape, seed, specs = case

    def kernel(s):
        if s["kind"] != "raw":
            return KernelSpec(**s).array()
        k = np.random.default_rng(s["seed"]).uniform(-0.2, 1.0, (s["size"], s["size"]))
        return (k / k.sum()).astype(np.float32)

    return inputs((2, 3, *shape), seed), np.stack([kernel(s) for s in specs])


def builder_ours(case):
    """our builder's float32 kernel for a BUILDER_CASES entry"""
    from resshift_amd import degrade

    _, fn, kw = case
    if fn == "circular_lowpass_kernel":
        return degrade.sinc_kernel(kw["cutoff"], kw["kernel_size"], kw["pad_to"])
    kind = {"bivariate_Gaussian": "", "bivariate_generalized_Gaussian": "generalized_", "bivariate_plateau": "plateau_"}[fn] + ("iso" if kw["isotropic"] else "aniso")
    return degrade.blur_kernel(kind, kw["kernel_size"], kw["sig_x"], kw["sig_y"], kw["theta"], kw.get("beta", 1.0))


# ---------------------------------------------------------------------------------------------------------------- filter2D
def reflect(q, n, repeat_edge=False):
    """torch's `reflect` (the edge sample is not repeated); repeat_edge: the symmetric reflection, a mutation"""
    q = np.asarray(q)
    if repeat_edge:
        return np.where(q < 0, -q - 1, np.where(q >= n, 2 * n - 1 - q, q))
    return np.where(q < 0, -q, np.where(q >= n, 2 * (n - 1) - q, q))


def filter2d(x, kernels, flip=False, repeat_edge=False):
    """out[b,c,i,j] = sum_{u,v} kernels[kb,u,v] x[b,c,refl(i + u - p),refl(j + v - p)], kb = 0 for one kernel, b for one per image"""
    x = np.asarray(x, np.float64)
    kernels = np.asarray(kernels, np.float64)
    B, C, H, W = x.shape
    Bk, k, _ = kernels.shape
    assert Bk in (1, B) and k % 2 == 1 and k // 2 < min(H, W)
    p = k // 2
    rows, cols = reflect(np.arange(-p, H + p), H, repeat_edge), reflect(np.arange(-p, W + p), W, repeat_edge)
    xp = x[:, :, rows][:, :, :, cols]
    out = np.zeros_like(x)
    for b in range(B):
        kb = kernels[0 if Bk == 1 else b]
        if flip:
            kb = kb[::-1, ::-1]
        for u in range(k):
            for v in range(k):
                out[b] += kb[u, v] * xp[b, :, u:u + H, v:v + W]
    return out


# ---------------------------------------------------------------------------------------------------------------- F.interpolate
def interpolate(x, scale_factor=None, size=None, mode="bilinear"):
    """F.interpolate on float64: the definition"""
    t = torch.from_numpy(np.asarray(x, np.float64))
    kw = dict(scale_factor=scale_factor) if scale_factor is not None else dict(size=tuple(size))
    if mode != "area":
        kw["align_corners"] = False
    return F.interpolate(t, mode=mode, **kw).numpy()


def out_size(n, scale_factor):
    return int(np.floor(float(n) * float(scale_factor)))


def _cubic_matrix(n, m, step, A):
    """[m, n]: row i holds the four weights of Keys' cubic around src = step (i + 0.5) - 0.5, indices clamped to the image"""
    M = np.zeros((m, n))
    c1 = lambda t: ((A + 2) * t - (A + 3)) * t * t + 1
    c2 = lambda t: ((A * t - 5 * A) * t + 8 * A) * t - 4 * A
    for i in range(m):
        src = step * (i + 0.5) - 0.5
        f = int(np.floor(src))
        t = src - f
        for j, w in zip(range(f - 1, f + 3), (c2(t + 1), c1(t), c1(1 - t), c2(2 - t))):
            M[i, min(max(j, 0), n - 1)] += w
    return M


def bicubic(x, scale_factor=None, size=None, A=-0.75, step_from_size=False):
    """the bicubic mode restated: A is Keys' constant; step_from_size takes the coordinates from H / Ho where a scale factor was given"""
    x = np.asarray(x, np.float64)
    H, W = x.shape[-2:]
    if scale_factor is not None:
        Ho, Wo = out_size(H, scale_factor), out_size(W, scale_factor)
        sh = sw = 1.0 / scale_factor
        if step_from_size:
            sh, sw = H / Ho, W / Wo
    else:
        Ho, Wo = size
        sh, sw = H / Ho, W / Wo
    return np.einsum("ih,bchw,jw->bcij", _cubic_matrix(H, Ho, sh, A), x, _cubic_matrix(W, Wo, sw, A))


# ---------------------------------------------------------------------------------------------------------------- DiffJPEG
def quality_to_factor(q):
    """the reference evaluates this on a float32 tensor; here: float64 of the float32 quality"""
    q = float(np.float32(q))
    return (5000.0 / q if q < 50 else 200.0 - 2.0 * q) / 100.0


def _blocks(plane):
    """[H, W] -> [H/8, W/8, 8, 8]"""
    H, W = plane.shape
    return plane.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3)


def _unblocks(b):
    nh, nw = b.shape[:2]
    return b.transpose(0, 2, 1, 3).reshape(nh * 8, nw * 8)


def dct(blocks):
    """F[u,v] = SCALE[u,v] sum_{x,y} f[x,y] cos((2x+1) u pi/16) cos((2y+1) v pi/16)"""
    return SCALE * np.einsum("...xy,xu,yv->...uv", blocks, COS, COS)


def idct(coef):
    """f[x,y] = 1/4 sum_{u,v} a[u] a[v] F[u,v] cos((2x+1) u pi/16) cos((2y+1) v pi/16) + 128"""
    return 0.25 * np.einsum("...uv,xu,yv->...xy", coef * ALPHA2, COS, COS) + 128.0


def jpeg_decode(qy, qcb, qcr, factor, H, W):
    """quantised coefficient blocks ([Hp/8,Wp/8,8,8] and two [Hp/16,Wp/16,8,8]) of one image -> RGB [3,H,W] in [0,1]"""
    y = _unblocks(idct(qy * (Y_TABLE * factor)))
    cb = np.repeat(np.repeat(_unblocks(idct(qcb * (C_TABLE * factor))), 2, 0), 2, 1)
    cr = np.repeat(np.repeat(_unblocks(idct(qcr * (C_TABLE * factor))), 2, 0), 2, 1)
    rgb = np.einsum("rc,chw->rhw", INV, np.stack([y, cb - 128.0, cr - 128.0]))
    return (np.clip(rgb, 0.0, 255.0) / 255.0)[:, :H, :W]


def jpeg(x, quality, half_away=False, subsample=True, chroma_table=True, replicate_pad=False, return_coefficients=False):
    """DiffJPEG(differentiable=False) of x [B,3,H,W] with one quality per image.  return_coefficients: also, per image, the PRE-round
    quantised coefficients (y [Hp/8,Wp/8,8,8], cb, cr [Hp/16,Wp/16,8,8]).  Mutations: rounding half away from zero, chroma not
    subsampled (kept at full resolution, its blocks quantised like chroma), the luma table for chroma, padding by replication."""
    x = np.asarray(x, np.float64)
    B, C, H, W = x.shape
    assert C == 3
    Hp, Wp = -(-H // 16) * 16, -(-W // 16) * 16
    rnd = (lambda v: np.sign(v) * np.floor(np.abs(v) + 0.5)) if half_away else np.rint
    out, coefs = np.empty_like(x), []
    for b in range(B):
        f = quality_to_factor(quality[b])
        img = np.pad(x[b], ((0, 0), (0, Hp - H), (0, Wp - W)), mode="edge" if replicate_pad else "constant") * 255.0
        ycc = np.einsum("rc,chw->rhw", FWD, img) + np.array([0.0, 128.0, 128.0])[:, None, None]
        ctab = (C_TABLE if chroma_table else Y_TABLE) * f
        cy = dct(_blocks(ycc[0]) - 128.0) / (Y_TABLE * f)
        if subsample:
            pool = lambda p: p.reshape(Hp // 2, 2, Wp // 2, 2).mean(axis=(1, 3))
            ccb, ccr = dct(_blocks(pool(ycc[1])) - 128.0) / ctab, dct(_blocks(pool(ycc[2])) - 128.0) / ctab
            out[b] = jpeg_decode(rnd(cy), rnd(ccb), rnd(ccr), f, H, W) if chroma_table else _decode_with(rnd(cy), rnd(ccb), rnd(ccr), f, ctab, H, W, True)
        else:
            ccb, ccr = dct(_blocks(ycc[1]) - 128.0) / ctab, dct(_blocks(ycc[2]) - 128.0) / ctab
            out[b] = _decode_with(rnd(cy), rnd(ccb), rnd(ccr), f, ctab, H, W, False)
        coefs.append((cy, ccb, ccr))
    return (out, coefs) if return_coefficients else out


def _decode_with(qy, qcb, qcr, factor, ctab, H, W, repeat):
    y = _unblocks(idct(qy * (Y_TABLE * factor)))
    cb, cr = _unblocks(idct(qcb * ctab)), _unblocks(idct(qcr * ctab))
    if repeat:
        cb, cr = np.repeat(np.repeat(cb, 2, 0), 2, 1), np.repeat(np.repeat(cr, 2, 0), 2, 1)
    rgb = np.einsum("rc,chw->rhw", INV, np.stack([y, cb - 128.0, cr - 128.0]))
    return (np.clip(rgb, 0.0, 255.0) / 255.0)[:, :H, :W]


def mcu_tie_distance(coefs):
    """[Hp/16, Wp/16]: per MCU of one image, the smallest distance of any of its pre-round coefficients from a half-integer"""
    cy, ccb, ccr = coefs
    d = lambda c: np.abs(np.abs(c - np.floor(c)) - 0.5).min(axis=(2, 3))
    dy = d(cy)
    dy = dy.reshape(dy.shape[0] // 2, 2, dy.shape[1] // 2, 2).min(axis=(1, 3))
    return np.minimum(dy, np.minimum(d(ccb), d(ccr)))


def constructed_jpeg_case(Hh, W, qualities, seed, qmax=6):
    """Inputs whose pre-round coefficients are known: per image, quantised coefficients q + u with integer q (|q| <= qmax at the lowest
    frequencies, thinning out towards the high ones) and u uniform in [-0.4, 0.4], dequantised, inverse-transformed in float64, chroma
    repeated 2 x 2, and mapped back to RGB with the exact inverse of the forward matrix.  The forward path of a correct codec then finds q
    + u again - every coefficient at least 0.1 from a rounding tie - and the expected output is the decode of q, in closed form.  Returns
    (x float32 [B,3,H,W] - not clamped, values may leave [0,1] slightly -, expected float64, the smallest tie distance of the float64
    forward path on the float32 input)."""
    assert Hh % 16 == 0 and W % 16 == 0
    rng = np.random.default_rng(seed)
    B = len(qualities)
    x, want = np.empty((B, 3, Hh, W), np.float32), np.empty((B, 3, Hh, W))
    fade = 1.0 / (1.0 + np.add.outer(np.arange(8), np.arange(8)))
    back = np.linalg.inv(FWD)
    for b, q in enumerate(qualities):
        f = quality_to_factor(q)

        def draw(nh, nw, table, dc):
            k = np.rint(rng.uniform(-qmax, qmax, (nh, nw, 8, 8)) * fade)
            k[..., 0, 0] = np.rint(rng.uniform(-dc, dc, (nh, nw)) / (table[0, 0] * f))     # (the mean level stays inside the pixel range)
            return k, k + rng.uniform(-0.4, 0.4, k.shape)

        ky, vy = draw(Hh // 8, W // 8, Y_TABLE, 300.0)
        kcb, vcb = draw(Hh // 16, W // 16, C_TABLE, 150.0)
        kcr, vcr = draw(Hh // 16, W // 16, C_TABLE, 150.0)
        y = _unblocks(idct(vy * (Y_TABLE * f)))
        up = lambda v: np.repeat(np.repeat(_unblocks(idct(v * (C_TABLE * f))), 2, 0), 2, 1)
        ycc = np.stack([y, up(vcb), up(vcr)]) - np.array([0.0, 128.0, 128.0])[:, None, None]
        x[b] = (np.einsum("rc,chw->rhw", back, ycc) / 255.0).astype(np.float32)
        want[b] = jpeg_decode(ky, kcb, kcr, f, Hh, W)
    _, coefs = jpeg(x, qualities, return_coefficients=True)
    return x, want, min(float(mcu_tie_distance(c).min()) for c in coefs)


# ---------------------------------------------------------------------------------------------------------------- noise, rounding
def add_noise(x, normals, sigma, gray, clamp=True):
    """x + sigma[b] / 255 n: normals[b] is [C,H,W], or [1,H,W] for an image whose gray flag is set (shared by its channels)"""
    out = np.array(x, np.float64)
    for b in range(out.shape[0]):
        n = np.asarray(normals[b], np.float64)
        assert n.shape[0] == (1 if gray[b] else out.shape[1])
        out[b] += float(sigma[b]) / 255.0 * n
    return np.clip(out, 0.0, 1.0) if clamp else out


def unit_to_u8(x):
    """[B,C,H,W] -> uint8 [B,H,W,C] = clamp(rint(x 255), 0, 255); rint of the FLOAT32 product, ties to even, as the kernel defines it"""
    v = np.asarray(x, np.float32) * np.float32(255.0)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1)


# ---------------------------------------------------------------------------------------------------------------- plan stages
def stage(plan, name, x, normals=None):
    """the float64 output of the operator call `name` of `plan` (resshift_amd.degrade.DegradePlan.stages) fed the input x [B,3,h,w];
    `normals`: for the noise stages, the per-image normal arrays (see add_noise).  `round` returns uint8 NHWC."""
    kernels = lambda specs: np.stack([s.array() for s in specs])
    size = (plan.H // plan.sf, plan.W // plan.sf)
    if name == "blur1":
        return filter2d(x, kernels(plan.first.kernels))
    if name == "resize1":
        return interpolate(x, scale_factor=plan.first.scale, mode=plan.first.mode)
    if name == "noise1":
        return add_noise(x, normals, plan.first.sigma, plan.first.gray)
    if name == "jpeg1":
        return jpeg(x, plan.jpeg1)
    if name == "blur2":
        return filter2d(x, kernels(plan.second.kernels))
    if name == "resize2":
        return interpolate(x, size=plan.second_size(), mode=plan.second.mode)
    if name == "noise2":
        return add_noise(x, normals, plan.second.sigma, plan.second.gray)
    if name == "resize3":
        return interpolate(x, size=size, mode=plan.final_mode)
    if name == "sinc":
        y = filter2d(x, kernels(plan.final_kernels))
        return np.clip(y, 0.0, 1.0) if plan.sinc_first else y
    if name == "jpeg2":
        return jpeg(x, plan.jpeg2)
    if name == "round":
        return unit_to_u8(x)
    raise KeyError(name)

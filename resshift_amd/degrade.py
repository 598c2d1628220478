"""On-device Real-ESRGAN degradation: LQ test sets from ground truth.

The reference makes the LQ inputs of its `realsr` benchmarks with scripts/prepare_testing_imagenet_sr.py -> RealESRGANDataset.degrade_fun
(basicsr/data/realesrgan_dataset.py:174-363) under configs/degradation_testing_realesrgan.yaml: blur, unantialiased resize, noise,
DiffJPEG and a sinc filter, on a CPU with cv2 / torchvision.  Here the random choices are made on the host, once, into a `DegradePlan`
(`draw_plan`), and a `Degrader` executes a plan on the device with the engine's operators (rs_filter2d, rs_interp, rs_add_noise,
rs_jpeg, rs_unit_to_u8).  `make_testset` turns a folder of ground-truth images into a folder of LQ PNGs plus plans.json, after which
`ResShiftSampler.inference(lq_dir, out, gt_path=gt_dir)` scores the restoration.  No sampler and no weights are needed.

    python -m resshift_amd.degrade GT_DIR LQ_DIR [--sf 4] [--seed 10000] [--recipe realesrgan | face]

The face recipe - scripts/prepare_testing_celeba_faceir.py -> datapipe/face_degradation_testing.py face_degradation: a
41-tap anisotropic Gaussian blur, a bilinear resize down by a real factor up to 32, noise, cv2's JPEG codec, a bilinear resize back -
is `FaceOptions` / `FacePlan` / `draw_face_plan` / `Degrader.run_face` / `make_face_testset` on rs_blur_resize and rs_jpeg_codec.

Not built: Poisson noise (`draw_plan` raises for gaussian_noise_prob < 1; the preset sets both to 1.0 where the
reference's recipe has 0.5), the ground truth's SmallestMaxSize + CenterCrop preparation, the reference's RNG stream.
"""
from __future__ import annotations

import dataclasses
import json
import math
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .continuous import request_seed
from .imageops import ImageOps

KERNEL_KINDS = ("iso", "aniso", "generalized_iso", "generalized_aniso", "plateau_iso", "plateau_aniso")
MODES = ("area", "bilinear", "bicubic")
IMAGE_EXTS = ("png", "jpg", "jpeg", "JPEG", "bmp")   # the listing of ResShiftSampler.inference


# ---------------------------------------------------------------------------------------------------------------- blur kernels
def _quadratic_form(size, sig_x, sig_y, theta, isotropic):
    """(x, y) Sigma^-1 (x, y)^T on the size x size grid centred at zero (basicsr/data/degradations.py mesh_grid, sigma_matrix2)"""
    ax = np.arange(-size // 2 + 1.0, size // 2 + 1.0)
    xx, yy = np.meshgrid(ax, ax)
    grid = np.stack([xx, yy], axis=-1)
    if isotropic:
        sigma = np.array([[sig_x ** 2, 0.0], [0.0, sig_x ** 2]])
    else:
        u = np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
        sigma = u @ np.diag([sig_x ** 2, sig_y ** 2]) @ u.T
    return np.sum((grid @ np.linalg.inv(sigma)) * grid, axis=2)


def blur_kernel(kind, size, sig_x, sig_y=None, theta=0.0, beta=1.0) -> np.ndarray:
    """float32 [size, size], sum 1: the reference's bivariate_Gaussian (`iso`, `aniso`), bivariate_generalized_Gaussian
    (`generalized_*`: exp(-q^beta / 2)) and bivariate_plateau (`plateau_*`: 1 / (q^beta + 1)) with q the quadratic form of the (rotated)
    covariance; computed in float64.  The `*_iso` kinds use sig_x only."""
    if kind not in KERNEL_KINDS:
        raise ValueError(f"unknown blur kernel {kind!r} (one of {KERNEL_KINDS})")
    if size % 2 != 1 or size < 1:
        raise ValueError(f"the kernel size must be odd, not {size}")
    q = _quadratic_form(int(size), float(sig_x), float(sig_x if sig_y is None else sig_y), float(theta), kind.endswith("_iso") or kind == "iso")
    if kind in ("iso", "aniso"):
        k = np.exp(-0.5 * q)
    elif kind.startswith("generalized"):
        k = np.exp(-0.5 * np.power(q, beta))
    else:
        k = np.reciprocal(np.power(q, beta) + 1.0)
    return (k / k.sum()).astype(np.float32)


def sinc_kernel(cutoff, size, pad_to=0) -> np.ndarray:
    """float32 2-D circular low-pass (sinc) filter of the reference's circular_lowpass_kernel: cutoff J1(cutoff r) / (2 pi r), cutoff^2 / (4 pi)
    at the centre, normalised to sum 1 (it has negative lobes), zero-padded to `pad_to`.  J1 is torch.special.bessel_j1 in float64."""
    if size % 2 != 1 or size < 1:
        raise ValueError(f"the kernel size must be odd, not {size}")
    c = (size - 1) / 2
    x, y = np.meshgrid(np.arange(size) - c, np.arange(size) - c, indexing="ij")
    r = np.sqrt(x ** 2 + y ** 2)
    r[(size - 1) // 2, (size - 1) // 2] = 1.0
    k = cutoff * torch.special.bessel_j1(torch.from_numpy(cutoff * r)).numpy() / (2 * np.pi * r)
    k[(size - 1) // 2, (size - 1) // 2] = cutoff ** 2 / (4 * np.pi)
    k = k / k.sum()
    if pad_to > size:
        p = (pad_to - size) // 2
        k = np.pad(k, ((p, p), (p, p)))
    return k.astype(np.float32)


def pad_kernel(k, pad_to) -> np.ndarray:
    p = (pad_to - k.shape[0]) // 2
    return np.pad(k, ((p, p), (p, p))) if p > 0 else k


@dataclass(frozen=True)
class KernelSpec:
    """a kernel by its parameters: `kind` one of KERNEL_KINDS, "sinc" (cutoff) or "pulse" (the identity); `size` padded with zeros to `pad_to`"""
    kind: str
    size: int
    pad_to: int
    sig_x: float = 0.0
    sig_y: float = 0.0
    theta: float = 0.0
    beta: float = 1.0
    cutoff: float = 0.0

    def array(self) -> np.ndarray:
        if self.kind == "pulse":
            k = np.zeros((self.pad_to, self.pad_to), np.float32)
            k[self.pad_to // 2, self.pad_to // 2] = 1.0
            return k
        if self.kind == "sinc":
            return sinc_kernel(self.cutoff, self.size, self.pad_to)
        return pad_kernel(blur_kernel(self.kind, self.size, self.sig_x, self.sig_y, self.theta, self.beta), self.pad_to)


# ---------------------------------------------------------------------------------------------------------------- options
@dataclass(frozen=True)
class DegradeOptions:
    """the `opts` and `degradation` sections of the reference's degradation YAML, under its field names"""
    blur_kernel_size: int
    kernel_list: Tuple[str, ...]
    kernel_prob: Tuple[float, ...]
    sinc_prob: float
    blur_sigma: Tuple[float, float]
    betag_range: Tuple[float, float]
    betap_range: Tuple[float, float]
    blur_kernel_size2: int
    kernel_list2: Tuple[str, ...]
    kernel_prob2: Tuple[float, ...]
    sinc_prob2: float
    blur_sigma2: Tuple[float, float]
    betag_range2: Tuple[float, float]
    betap_range2: Tuple[float, float]
    final_sinc_prob: float
    sf: int
    resize_prob: Tuple[float, float, float]          # up, down, keep
    resize_range: Tuple[float, float]
    gaussian_noise_prob: float
    noise_range: Tuple[float, float]
    poisson_scale_range: Tuple[float, float]
    gray_noise_prob: float
    jpeg_range: Tuple[float, float]
    second_order_prob: float
    second_blur_prob: float
    resize_prob2: Tuple[float, float, float]
    resize_range2: Tuple[float, float]
    gaussian_noise_prob2: float
    noise_range2: Tuple[float, float]
    poisson_scale_range2: Tuple[float, float]
    gray_noise_prob2: float
    jpeg_range2: Tuple[float, float]


# configs/degradation_testing_realesrgan.yaml, except the two gaussian_noise_prob (0.5 there: Poisson noise is not built)
REALESRGAN_TESTING = DegradeOptions(
    blur_kernel_size=13, kernel_list=KERNEL_KINDS, kernel_prob=(0.60, 0.40, 0.0, 0.0, 0.0, 0.0), sinc_prob=0.1, blur_sigma=(0.2, 0.8),
    betag_range=(1.0, 1.5), betap_range=(1, 1.2),
    blur_kernel_size2=7, kernel_list2=KERNEL_KINDS, kernel_prob2=(0.60, 0.4, 0.0, 0.0, 0.0, 0.0), sinc_prob2=0.0, blur_sigma2=(0.2, 0.5),
    betag_range2=(0.5, 0.8), betap_range2=(1, 1.2), final_sinc_prob=0.2,
    sf=4, resize_prob=(0.2, 0.7, 0.1), resize_range=(0.5, 1.5), gaussian_noise_prob=1.0, noise_range=(1, 15), poisson_scale_range=(0.05, 0.3),
    gray_noise_prob=0.4, jpeg_range=(70, 95),
    second_order_prob=0.0, second_blur_prob=0.2, resize_prob2=(0.3, 0.4, 0.3), resize_range2=(0.8, 1.2), gaussian_noise_prob2=1.0,
    noise_range2=(1, 10), poisson_scale_range2=(0.05, 0.2), gray_noise_prob2=0.4, jpeg_range2=(80, 100))


# ---------------------------------------------------------------------------------------------------------------- plans
@dataclass(frozen=True)
class StagePlan:
    """blur -> resize -> noise of one degradation order.  Shared by the batch: `scale`, `mode`; per image: `kernels` (None: no blur),
    `sigma`, `gray`"""
    kernels: Optional[Tuple[KernelSpec, ...]]
    scale: float
    mode: str
    sigma: Tuple[float, ...]
    gray: Tuple[bool, ...]


@dataclass(frozen=True)
class DegradePlan:
    """every random choice of one degrade_fun call on a batch of B ground-truth images of H x W"""
    B: int
    H: int
    W: int
    sf: int
    seed: int
    first: StagePlan                       # its resize takes scale_factor=first.scale
    jpeg1: Tuple[float, ...]
    second: Optional[StagePlan]            # its resize takes size=(int(H / sf * scale), int(W / sf * scale))
    sinc_first: bool                       # [resize back + sinc filter] before the last JPEG (else after it)
    final_mode: str
    final_kernels: Tuple[KernelSpec, ...]
    jpeg2: Tuple[float, ...]
    noise_seeds: Tuple[int, ...]           # image b's noise is noise_fill((noise_seeds[b], 0), draw = 0 (first) | 1 (second), ...)

    def second_size(self) -> Tuple[int, int]:
        return int(self.H / self.sf * self.second.scale), int(self.W / self.sf * self.second.scale)

    def stages(self) -> list:
        """the names of the operator calls, in order"""
        s = ["blur1", "resize1", "noise1", "jpeg1"]
        if self.second is not None:
            s += (["blur2"] if self.second.kernels is not None else []) + ["resize2", "noise2"]
        s += ["resize3", "sinc", "jpeg2"] if self.sinc_first else ["jpeg2", "resize3", "sinc"]
        return s + ["round"]

    def to_dict(self) -> dict:
        return dataclasses.asdict(self)

    def to_json(self) -> str:
        return json.dumps(self.to_dict())

    @staticmethod
    def from_dict(d) -> "DegradePlan":
        spec = lambda k: KernelSpec(**k)
        specs = lambda ks: None if ks is None else tuple(spec(k) for k in ks)
        stage = lambda s: None if s is None else StagePlan(kernels=specs(s["kernels"]), scale=float(s["scale"]), mode=s["mode"],
                                                           sigma=tuple(float(v) for v in s["sigma"]), gray=tuple(bool(v) for v in s["gray"]))
        return DegradePlan(B=int(d["B"]), H=int(d["H"]), W=int(d["W"]), sf=int(d["sf"]), seed=int(d["seed"]), first=stage(d["first"]),
                           jpeg1=tuple(float(v) for v in d["jpeg1"]), second=stage(d["second"]), sinc_first=bool(d["sinc_first"]),
                           final_mode=d["final_mode"], final_kernels=specs(d["final_kernels"]), jpeg2=tuple(float(v) for v in d["jpeg2"]),
                           noise_seeds=tuple(int(v) for v in d["noise_seeds"]))

    @staticmethod
    def from_json(text) -> "DegradePlan":
        return DegradePlan.from_dict(json.loads(text))


QUALITY_MAX = float(np.nextafter(np.float32(100.0), np.float32(0.0)))   # rs_jpeg takes qualities in (0, 100) as fp32


def _draw_kernel(rng, sizes, pad_to, sinc_prob, kinds, probs, sigma, betag, betap) -> KernelSpec:
    """the dataset's kernel drawing (realesrgan_dataset.py:174-218, degradations.py random_mixed_kernels)"""
    size = int(rng.choice(sizes))
    if rng.uniform() < sinc_prob:
        lo = np.pi / 3 if size < 13 else np.pi / 5
        return KernelSpec("sinc", size, pad_to, cutoff=float(rng.uniform(lo, np.pi)))
    kind = str(rng.choice(list(kinds), p=np.asarray(probs, np.float64) / np.sum(probs)))
    sig_x = float(rng.uniform(*sigma))
    sig_y, theta, beta = sig_x, 0.0, 1.0
    if kind.endswith("aniso"):
        sig_y, theta = float(rng.uniform(*sigma)), float(rng.uniform(-math.pi, math.pi))
    if kind.startswith(("generalized", "plateau")):
        lo, hi = betag if kind.startswith("generalized") else betap
        # (the reference assumes lo < 1 < hi; where its YAML has hi < 1 numpy's legacy uniform(1, hi) still draws between the two: so does this)
        u = rng.uniform()
        beta = float(lo + (1.0 - lo) * rng.random()) if u < 0.5 else float(1.0 + (hi - 1.0) * rng.random())
    return KernelSpec(kind, size, pad_to, sig_x=sig_x, sig_y=sig_y, theta=theta, beta=beta)


def _draw_stage(rng, B, kernels, probs, rng_range, noise_range, gray_prob) -> StagePlan:
    updown = str(rng.choice(["up", "down", "keep"], p=np.asarray(probs, np.float64) / np.sum(probs)))
    scale = float(rng.uniform(1.0, rng_range[1])) if updown == "up" else float(rng.uniform(rng_range[0], 1.0)) if updown == "down" else 1.0
    mode = str(rng.choice(MODES))
    sigma = tuple(float(rng.uniform(*noise_range)) for _ in range(B))
    gray = tuple(bool(rng.uniform() < gray_prob) for _ in range(B))
    return StagePlan(kernels=kernels, scale=scale, mode=mode, sigma=sigma, gray=gray)


def _quality(rng, lo_hi) -> float:
    return min(float(np.float32(rng.uniform(*lo_hi))), QUALITY_MAX)   # (uniform on [80, 100) can round to 100.0 in fp32)


def draw_plan(opts: DegradeOptions, B: int, H: int, W: int, seed: int) -> DegradePlan:
    """Every random choice of the reference's degrade_fun and of its dataset's kernel drawing, for a batch of B images of H x W, from
    numpy.random.Generator(Philox(seed)): equal arguments give equal plans, on any machine.  Shared by the batch (as in degrade_fun):
    resize direction / scale / mode per order, the second-order and second-blur flags, the order of the last JPEG and [resize back +
    sinc]; per image: kernel1, kernel2, sinc-or-pulse, sigma and gray flag per order, quality per JPEG, the noise seed.
    This is NOT the reference's RNG stream (Python's `random`, numpy's global state and torch's generator interleaved): the
    distribution is the recipe's, the draws are not."""
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"draw_plan: B, H and W must be positive, not {B}, {H}, {W}")
    for name in ("gaussian_noise_prob", "gaussian_noise_prob2"):
        if getattr(opts, name) < 1:
            raise ValueError(f"draw_plan: {name} = {getattr(opts, name)} asks for Poisson noise, which is not built (only Gaussian: set it to 1.0)")
    sf = int(opts.sf)
    if H % sf or W % sf:
        raise ValueError(f"draw_plan: {H} x {W} is no multiple of sf = {sf}")
    if opts.blur_kernel_size > _lib.FILTER_KMAX or opts.blur_kernel_size2 > _lib.FILTER_KMAX:
        raise ValueError(f"draw_plan: kernels above {_lib.FILTER_KMAX} taps are not supported")
    lo1 = min(1.0, opts.resize_range[0])
    if opts.blur_kernel_size // 2 >= min(H, W) or opts.blur_kernel_size2 // 2 >= min(H // sf, W // sf) \
            or opts.blur_kernel_size2 // 2 >= int(min(H, W) * lo1):
        raise ValueError(f"draw_plan: {H} x {W} is too small for the blur kernels ({opts.blur_kernel_size}, {opts.blur_kernel_size2} taps at 1 / {sf})")
    rng = np.random.Generator(np.random.Philox(int(seed) % 2 ** 64))
    sizes1, sizes2 = list(range(3, opts.blur_kernel_size, 2)), list(range(3, opts.blur_kernel_size2, 2))
    k1 = tuple(_draw_kernel(rng, sizes1, opts.blur_kernel_size, opts.sinc_prob, opts.kernel_list, opts.kernel_prob, opts.blur_sigma,
                            opts.betag_range, opts.betap_range) for _ in range(B))
    k2 = tuple(_draw_kernel(rng, sizes2, opts.blur_kernel_size2, opts.sinc_prob2, opts.kernel_list2, opts.kernel_prob2, opts.blur_sigma2,
                            opts.betag_range2, opts.betap_range2) for _ in range(B))
    final = []
    for _ in range(B):
        if rng.uniform() < opts.final_sinc_prob:
            size = int(rng.choice(sizes2))
            final.append(KernelSpec("sinc", size, opts.blur_kernel_size2, cutoff=float(rng.uniform(np.pi / 3, np.pi))))
        else:
            final.append(KernelSpec("pulse", opts.blur_kernel_size2, opts.blur_kernel_size2))
    first = _draw_stage(rng, B, k1, opts.resize_prob, opts.resize_range, opts.noise_range, opts.gray_noise_prob)
    jpeg1 = tuple(_quality(rng, opts.jpeg_range) for _ in range(B))
    second = None
    if rng.uniform() < opts.second_order_prob:
        blur2 = bool(rng.uniform() < opts.second_blur_prob)
        second = _draw_stage(rng, B, k2 if blur2 else None, opts.resize_prob2, opts.resize_range2, opts.noise_range2, opts.gray_noise_prob2)
    sinc_first = bool(rng.uniform() < 0.5)
    final_mode = str(rng.choice(MODES))
    jpeg2 = tuple(_quality(rng, opts.jpeg_range2) for _ in range(B))
    noise_seeds = tuple(int(v) for v in rng.integers(0, 2 ** 63, size=B))
    return DegradePlan(B=B, H=H, W=W, sf=sf, seed=int(seed), first=first, jpeg1=jpeg1, second=second, sinc_first=sinc_first,
                       final_mode=final_mode, final_kernels=tuple(final), jpeg2=jpeg2, noise_seeds=noise_seeds)


# ---------------------------------------------------------------------------------------------------------------- the face recipe
@dataclass(frozen=True)
class FaceOptions:
    """the ranges scripts/prepare_testing_celeba_faceir.py draws from (uniform on [lo, hi)), and face_degradation's kernel size"""
    sf: Tuple[float, float] = (1.0, 32.0)
    qf: Tuple[float, float] = (30.0, 70.0)
    nf: Tuple[float, float] = (1.0, 20.0)
    sig: Tuple[float, float] = (4.0, 16.0)
    theta: Tuple[float, float] = (0.0, math.pi)
    kernel_size: int = 41


FACE_TESTING = FaceOptions()
FACE_MIN_SIDE = 256   # below it `small` = side // sf can fall under rs_jpeg_codec's 8 at sf = 32


@dataclass(frozen=True)
class FacePlan:
    """every random choice of one face_degradation call on an image of H x W; `quality` = int(qf), which is what cv2 receives; `small` =
    (int(H // sf), int(W // sf)), the size between the two resizes"""
    H: int
    W: int
    sf: float
    sig_x: float
    sig_y: float
    theta: float
    nf: float
    quality: int
    small: Tuple[int, int]
    kernel_size: int
    seed: int
    noise_seed: int

    def stages(self) -> list:
        return ["blur_down", "noise", "jpeg", "up", "round"]

    def kernel(self) -> np.ndarray:
        return blur_kernel("aniso", self.kernel_size, self.sig_x, self.sig_y, self.theta)

    def to_dict(self) -> dict:
        return dataclasses.asdict(self)

    def to_json(self) -> str:
        return json.dumps(self.to_dict())

    @staticmethod
    def from_dict(d) -> "FacePlan":
        return FacePlan(H=int(d["H"]), W=int(d["W"]), sf=float(d["sf"]), sig_x=float(d["sig_x"]), sig_y=float(d["sig_y"]), theta=float(d["theta"]),
                        nf=float(d["nf"]), quality=int(d["quality"]), small=(int(d["small"][0]), int(d["small"][1])),
                        kernel_size=int(d["kernel_size"]), seed=int(d["seed"]), noise_seed=int(d["noise_seed"]))

    @staticmethod
    def from_json(text) -> "FacePlan":
        return FacePlan.from_dict(json.loads(text))


def face_plan(H, W, sf, sig_x, sig_y, theta, nf, qf, kernel_size=41, seed=0, noise_seed=0) -> FacePlan:
    """a FacePlan from face_degradation's own arguments: quality and small are derived as the reference derives them"""
    H, W, k = int(H), int(W), int(kernel_size)
    if H < 1 or W < 1:
        raise ValueError(f"face_plan: H and W must be positive, not {H}, {W}")
    if not 1.0 <= float(sf) <= 64.0:
        raise ValueError(f"face_plan: sf = {sf} must lie in [1, 64]")
    if k % 2 != 1 or not 1 <= k <= _lib.BLUR_RESIZE_KMAX:
        raise ValueError(f"face_plan: the kernel size must be odd and at most {_lib.BLUR_RESIZE_KMAX}, not {k}")
    if k // 2 >= min(H, W):
        raise ValueError(f"face_plan: {H} x {W} is too small for a blur kernel of {k} taps")
    quality, small = int(qf), (int(H // float(sf)), int(W // float(sf)))
    if not 1 <= quality <= 100:
        raise ValueError(f"face_plan: int(qf) = {quality} must lie in 1 .. 100")
    if min(small) < _lib.JPEG_CODEC_MIN:
        raise ValueError(f"face_plan: {H} x {W} at sf = {sf} gives {small[0]} x {small[1]}, below the JPEG codec's {_lib.JPEG_CODEC_MIN}")
    if not (float(nf) >= 0 and float(sig_x) > 0 and float(sig_y) > 0):
        raise ValueError(f"face_plan: nf must not be negative and the sigmas must be positive, not {nf}, {sig_x}, {sig_y}")
    return FacePlan(H=H, W=W, sf=float(sf), sig_x=float(sig_x), sig_y=float(sig_y), theta=float(theta), nf=float(nf), quality=quality, small=small,
                    kernel_size=k, seed=int(seed), noise_seed=int(noise_seed))


def draw_face_plan(opts: FaceOptions, H: int, W: int, seed: int) -> FacePlan:
    """The random choices of scripts/prepare_testing_celeba_faceir.py for one image, from numpy.random.Generator(Philox(seed)) in the
    script's order - sf, qf, nf, sig_x, sig_y, theta - then the noise seed.  As `draw_plan`: the recipe's distribution, not the
    reference's RNG stream (Python's `random`)."""
    if min(int(H), int(W)) < FACE_MIN_SIDE:
        raise ValueError(f"draw_face_plan: {H} x {W} has a side below {FACE_MIN_SIDE} (H // sf can fall under the JPEG codec's {_lib.JPEG_CODEC_MIN})")
    rng = np.random.Generator(np.random.Philox(int(seed) % 2 ** 64))
    sf, qf, nf = (float(rng.uniform(*r)) for r in (opts.sf, opts.qf, opts.nf))
    sig_x, sig_y, theta = (float(rng.uniform(*r)) for r in (opts.sig, opts.sig, opts.theta))
    return face_plan(H, W, sf, sig_x, sig_y, theta, nf, qf, opts.kernel_size, seed=seed, noise_seed=int(rng.integers(0, 2 ** 63)))


# ---------------------------------------------------------------------------------------------------------------- execution
class Degrader:
    """Executes DegradePlans on the device.  `engine_or_device`: an Engine (its filter2d / interpolate / jpeg / add_noise / unit_to_u8 are
    used), a device, or None for the current one."""

    def __init__(self, engine_or_device=None):
        self.ops = engine_or_device if hasattr(engine_or_device, "filter2d") else ImageOps(engine_or_device)
        self.device = self.ops.device

    def _kernels(self, specs):
        return torch.from_numpy(np.stack([s.array() for s in specs])).to(self.device)

    def _finish(self, x, log, trace):
        """the `round` stage and what `run` / `run_face` return"""
        u8 = self.ops.unit_to_u8(x)
        log.append(("round", x, u8))
        lq = u8.permute(0, 3, 1, 2).to(torch.float32).div(255.0).contiguous()
        return (lq, log) if trace else lq

    def run(self, gt01, plan: DegradePlan, trace=False):
        """gt01 [B,3,H,W] in [0,1] -> the LQ batch [B,3,H // sf,W // sf], fp32 in [0,1] on the 1/255 grid, in degrade_fun's order:
        blur -> resize -> noise (clamped) -> JPEG;  if drawn, the second order's (blur ->) resize -> noise (clamped);  then either order of
        JPEG and [resize to (H // sf, W // sf) + sinc filter] - whatever precedes a JPEG is clamped to [0, 1] - and the final clamp / round.
        `uint8()` of the result is exact.  trace=True: (lq, [(stage name, input, output)]) with the device tensors of every operator call,
        names as `plan.stages()`; the `round` stage's output is the uint8 NHWC tensor."""
        if tuple(gt01.shape) != (plan.B, 3, plan.H, plan.W):
            raise ValueError(f"Degrader.run: the plan is for {(plan.B, 3, plan.H, plan.W)}, the batch is {tuple(gt01.shape)}")
        ops, log = self.ops, []

        def step(name, x, y):
            log.append((name, x, y))
            return y

        keys = [(s, 0) for s in plan.noise_seeds]
        x = gt01.to(self.device, torch.float32).contiguous()
        f = plan.first
        x = step("blur1", x, ops.filter2d(x, self._kernels(f.kernels)))
        x = step("resize1", x, ops.interpolate(x, scale_factor=f.scale, mode=f.mode))
        x = step("noise1", x, ops.add_noise(x, keys, f.sigma, gray=f.gray, draw=0, clamp=True))
        x = step("jpeg1", x, ops.jpeg(x, plan.jpeg1))
        s = plan.second
        if s is not None:
            if s.kernels is not None:
                x = step("blur2", x, ops.filter2d(x, self._kernels(s.kernels)))
            x = step("resize2", x, ops.interpolate(x, size=plan.second_size(), mode=s.mode))
            x = step("noise2", x, ops.add_noise(x, keys, s.sigma, gray=s.gray, draw=1, clamp=True))
        size = (plan.H // plan.sf, plan.W // plan.sf)
        sinc = self._kernels(plan.final_kernels)
        if plan.sinc_first:
            x = step("resize3", x, ops.interpolate(x, size=size, mode=plan.final_mode))
            x = step("sinc", x, ops.filter2d(x, sinc, clamp=True))          # (the clamp in front of the JPEG)
            x = step("jpeg2", x, ops.jpeg(x, plan.jpeg2))
        else:
            x = step("jpeg2", x, ops.jpeg(x, plan.jpeg2))                   # (its input is a JPEG's or a clamped noise stage's output)
            x = step("resize3", x, ops.interpolate(x, size=size, mode=plan.final_mode))
            x = step("sinc", x, ops.filter2d(x, sinc))
        return self._finish(x, log, trace)

    def run_u8(self, gt_u8, plan: DegradePlan):
        """uint8 [B,H,W,3] -> uint8 [B,H // sf,W // sf,3] (device tensors): what `make_testset` reads and writes"""
        gt01 = gt_u8.to(self.device).permute(0, 3, 1, 2).to(torch.float32).div(255.0).contiguous()
        _, log = self.run(gt01, plan, trace=True)
        return log[-1][2]

    def run_face(self, gt01, plan: FacePlan, trace=False):
        """gt01 [1,3,H,W] in [0,1], RGB -> the face LQ image [1,3,H,W], fp32 on the 1/255 grid, in face_degradation's order: `blur_down` (the
        41-tap Gaussian under the bilinear resize to plan.small, one launch), `noise` (clamped), `jpeg` (libjpeg's codec at plan.quality),
        `up` (the bilinear resize back to H x W), `round`.  One image per call: `small` differs from image to image.  trace=True: (lq,
        [(stage, input, output)]) as `run` returns it."""
        if tuple(gt01.shape) != (1, 3, plan.H, plan.W):
            raise ValueError(f"Degrader.run_face: the plan is for {(1, 3, plan.H, plan.W)}, the batch is {tuple(gt01.shape)}")
        ops, log = self.ops, []

        def step(name, x, y):
            log.append((name, x, y))
            return y

        x = gt01.to(self.device, torch.float32).contiguous()
        kernel = torch.from_numpy(plan.kernel()[None]).to(self.device)
        x = step("blur_down", x, ops.blur_resize(x, kernel, tuple(plan.small)))
        x = step("noise", x, ops.add_noise(x, [(plan.noise_seed, 0)], [plan.nf], gray=False, draw=0, clamp=True))
        x = step("jpeg", x, ops.jpeg_codec(x, [plan.quality]))
        x = step("up", x, ops.blur_resize(x, None, (plan.H, plan.W)))
        return self._finish(x, log, trace)

    def run_face_u8(self, gt_u8, plan: FacePlan):
        """uint8 [1,H,W,3] -> uint8 [1,H,W,3] (device tensors): what `make_face_testset` reads and writes"""
        gt01 = gt_u8.to(self.device).permute(0, 3, 1, 2).to(torch.float32).div(255.0).contiguous()
        _, log = self.run_face(gt01, plan, trace=True)
        return log[-1][2]


# ---------------------------------------------------------------------------------------------------------------- files
def list_images(path) -> list:
    """the files of a directory as ResShiftSampler.inference lists them (one recursive glob per extension, each sorted); a file is itself"""
    path = Path(path)
    if not path.is_dir():
        return [path]
    return [p for e in IMAGE_EXTS for p in sorted(path.glob(f"**/*.{e}"))]


FILES_KEY = "_files"   # plans.json: how the LQ files were written, where that is not the default PNG


def write_plans(lq_dir, plans, ext="png", quality=None) -> None:
    """lq_dir/plans.json: {stem: plan as a dict}, sorted by stem; for JPEG files also {"_files": {"ext": "jpg", "quality": q}}"""
    table = {k: p.to_dict() for k, p in sorted(plans.items())}
    if ext != "png":
        table[FILES_KEY] = {"ext": ext, "quality": quality}
    with open(Path(lq_dir) / "plans.json", "w") as fh:
        json.dump(table, fh, indent=1)


def _file_format(ext, quality):
    """(ext, quality) of the LQ files: "png", or "jpg" with an integer quality 1 .. 100 (default 95)"""
    if ext not in ("png", "jpg"):
        raise ValueError(f"ext must be 'png' or 'jpg', not {ext!r}")
    if ext == "png":
        if quality is not None:
            raise ValueError("quality belongs to ext='jpg'")
        return ext, None
    quality = 95 if quality is None else quality
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError(f"quality must be an integer in 1 .. 100, not {quality!r}")
    return ext, quality


def _make_set(gt_dir, lq_dir, size_error, plan_for, run_u8, device, seed, positions, ext="png", quality=None) -> dict:
    """what `make_testset` and `make_face_testset` share.  size_error(h, w): None, or why the recipe does not take an image of that size;
    plan_for(h, w, seed): the image's plan; run_u8(degrader, uint8 [1,H,W,3], plan): its LQ image, uint8 [1,h,w,3] on the device.
    ext="jpg": the LQ image is written as a real JPEG at `quality`, coded on the device (ImageOps.jpeg_encode)."""
    from PIL import Image

    ext, quality = _file_format(ext, quality)
    files = list_images(gt_dir)
    todo = list(range(len(files))) if positions is None else list(positions)
    sizes = {}
    for i in todo:
        with Image.open(files[i]) as im:
            w, h = im.size
        why = size_error(h, w)
        if why:
            raise ValueError(f"{files[i]}: {h} x {w} {why}")
        sizes[i] = (h, w)
    lq_dir = Path(lq_dir)
    lq_dir.mkdir(parents=True, exist_ok=True)
    dg = Degrader(device)
    plans = {}
    for i in todo:
        plan = plan_for(*sizes[i], request_seed(seed, i))
        gt = torch.from_numpy(np.asarray(Image.open(files[i]).convert("RGB"), dtype=np.uint8).copy()).unsqueeze(0)
        lq = run_u8(dg, gt, plan)
        if ext == "png":
            Image.fromarray(lq[0].cpu().numpy()).save(lq_dir / f"{files[i].stem}.png")
        else:
            (lq_dir / f"{files[i].stem}.jpg").write_bytes(dg.ops.jpeg_encode(lq, quality)[0])
        plans[files[i].stem] = plan
    if positions is None:
        write_plans(lq_dir, plans, ext, quality)
    return plans


def make_testset(gt_dir, lq_dir, sf=4, opts: DegradeOptions = REALESRGAN_TESTING, seed=10000, device=None, positions=None, ext="png",
                 quality=None) -> dict:
    """A folder of ground-truth images -> lq_dir/<stem>.png, degraded on the device, plus lq_dir/plans.json {stem: plan}.  The image at
    position i of the sorted listing gets one plan with B = 1 from the seed continuous.request_seed(seed, i): a file's LQ image depends
    on its position and the seed only.  Every side of every image must be a multiple of `sf` (ValueError naming the file, before
    anything is written).  `device`: a device or an Engine.  `positions` (of the listing; default: all of it): the files this call
    degrades - the caller then writes plans.json itself (`write_plans`) from what its ranks return.  `ext="jpg"`: lq_dir/<stem>.jpg
    instead, real JPEG files at `quality` (1 .. 100, default 95) coded on the device; plans.json records both.  Returns {stem: DegradePlan}."""
    opts = dataclasses.replace(opts, sf=int(sf))
    return _make_set(gt_dir, lq_dir, lambda h, w: f"is no multiple of sf = {opts.sf}" if h % opts.sf or w % opts.sf else None,
                     lambda h, w, s: draw_plan(opts, 1, h, w, s), lambda dg, gt, plan: dg.run_u8(gt, plan), device, seed, positions, ext, quality)


def make_face_testset(gt_dir, lq_dir, opts: FaceOptions = FACE_TESTING, seed=10000, device=None, positions=None) -> dict:
    """`make_testset` for the face recipe: lq_dir/<stem>.png of the GROUND TRUTH'S size plus lq_dir/plans.json {stem: FacePlan}; the image at
    position i of the sorted listing gets the plan draw_face_plan(opts, H, W, request_seed(seed, i)).  Every side must be at least 256
    (ValueError naming the file, before anything is written).  `device`, `positions` and the return value as `make_testset` has them."""
    return _make_set(gt_dir, lq_dir, lambda h, w: f"has a side below {FACE_MIN_SIDE}" if min(h, w) < FACE_MIN_SIDE else None,
                     lambda h, w, s: draw_face_plan(opts, h, w, s), lambda dg, gt, plan: dg.run_face_u8(gt, plan), device, seed, positions)


def main(argv=None):
    import argparse

    ap = argparse.ArgumentParser(prog="python -m resshift_amd.degrade", description="Real-ESRGAN or face degradation of a folder of ground-truth images, on the device")
    ap.add_argument("gt_dir")
    ap.add_argument("lq_dir")
    ap.add_argument("--sf", type=int, default=4)
    ap.add_argument("--seed", type=int, default=10000)
    ap.add_argument("--recipe", choices=("realesrgan", "face"), default="realesrgan",
                    help="face: datapipe/face_degradation_testing.py (the LQ images keep the ground truth's size; --sf is not used)")
    ap.add_argument("--ext", choices=("png", "jpg"), default="png", help="jpg (realesrgan recipe): the LQ files are JPEGs coded on the device")
    ap.add_argument("--quality", type=int, default=None, help="the JPEG quality of --ext jpg, 1 .. 100 (default 95)")
    a = ap.parse_args(argv)
    if a.recipe == "face":
        if a.ext != "png" or a.quality is not None:
            ap.error("--ext / --quality belong to the realesrgan recipe")
        plans = make_face_testset(a.gt_dir, a.lq_dir, seed=a.seed)
    else:
        fmt = {} if a.ext == "png" and a.quality is None else dict(ext=a.ext, quality=a.quality)
        plans = make_testset(a.gt_dir, a.lq_dir, sf=a.sf, seed=a.seed, **fmt)
    print(f"{len(plans)} images -> {a.lq_dir} (plans.json)")


if __name__ == "__main__":
    main()

"""Float64 restatement of rs_blur_resize (include/resshift_hip.h "face degradation"): tests/_degrade_ref.py's filter2d
followed by F.interpolate(mode="bilinear", align_corners=False) on float64 - the two definitions, composed - and the execution of a
FacePlan stage."""
import numpy as np

import _degrade_ref as D
import _jpeg_ref as J

# The distance of the reference's OWN fp32 filter2D -> fp32 F.interpolate(bilinear) from this restatement on BLUR_CASES, as
# tests/test_face_degrade_cpu.py measures it from tests/golden/reference_face.npz (it asserts that the measurement lies in (REF_ERR / 2,
# REF_ERR]); the GPU bound is five times this, absolute, on every element (DESIGN.md 7f's rule).
REF_ERR = 2.0e-6
TOL = 5.0 * REF_ERR

# (key, kernel size, kernels: 1 shared | 2 per image, kernel seed): seeded random kernels with sum 1 - a Gaussian equals its own flip and
# could not catch a flipped kernel.  Inputs: D.inputs((2, 3, *BLUR_SHAPE), BLUR_SEED + index).
BLUR_SHAPE, BLUR_SEED = (45, 52), 71
BLUR_SIZES = [(45, 52), (11, 13), (1, 2), (23, 31)]     # equal size, a step of 4, a step of 45 / 26, a step of nearly 2 (the LDS-staged kernel's largest)
GPU_EXTRA_SIZES = [(60, 70), (11, 31)]                   # not recorded: an enlargement under the blur; one axis on either side of the kernels' switch
BLUR_KERNELS = [("k41_shared", 41, 1, 81), ("k41_per_image", 41, 2, 82), ("k21_shared", 21, 1, 83), ("k21_per_image", 21, 2, 84),
                ("k3_shared", 3, 1, 85), ("k3_per_image", 3, 2, 86)]
#   without a kernel: (input shape, output size) - a ratio of 32 and a fractional one.  Inputs: D.inputs((2, 3, *shape), RESIZE_SEED + index);
#   the fixture records the first plane only (the ratio-32 output is large)
RESIZE_CASES = [((6, 10), (192, 320)), ((24, 40), (31, 47))]
RESIZE_SEED = 91


def raw_kernels(k, n, seed):
    ks = np.random.default_rng(seed).uniform(-0.2, 1.0, (n, k, k))
    return (ks / ks.sum(axis=(1, 2), keepdims=True)).astype(np.float32)


def blur_case(index):
    """(x float32 [2,3,45,52], kernels float32 [1 | 2,k,k]) of BLUR_KERNELS[index]"""
    _, k, n, seed = BLUR_KERNELS[index]
    return D.inputs((2, 3, *BLUR_SHAPE), BLUR_SEED + index), raw_kernels(k, n, seed)


def blur_resize(x, kernels, size, flip=False):
    y = np.asarray(x, np.float64) if kernels is None else D.filter2d(x, kernels, flip=flip)
    return D.interpolate(y, size=tuple(size), mode="bilinear")


def stage(plan, name, x, normals=None):
    """the output of the operator call `name` of a resshift_amd.degrade.FacePlan fed the input x [1,3,h,w]: float64, except `jpeg` (the
    exact float32 result) and `round` (uint8 NHWC)"""
    if name == "blur_down":
        return blur_resize(x, plan.kernel()[None], plan.small)
    if name == "noise":
        return D.add_noise(x, normals, [plan.nf], [False])
    if name == "jpeg":
        return J.codec(np.asarray(x, np.float32), [plan.quality])
    if name == "up":
        return blur_resize(x, None, (plan.H, plan.W))
    if name == "round":
        return D.unit_to_u8(x)
    raise KeyError(name)

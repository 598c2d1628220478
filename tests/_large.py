"""What tests/test_large_tensors_gpu.py and tests/test_large_tensors_cpu.py share: the case tables of the tensors past 2^31 bytes, the
periodic operands and the chunked comparison.

A large operand is P = 3 distinct images repeated along the batch: the float64 reference costs three images and every image b of a result
is compared with ref[b % 3].  An address that lost bit 31, wrapped at 2^32 or went through an `int` lands 2^31 or 2^32 bytes away; it reads
the same data only if that distance is a whole number of periods, which `alias_visible` rules out for every operand (3 divides no power of
two, so it holds for any image size - the CPU test asserts it case by case all the same)."""
import gc
import math
import zlib
from collections import namedtuple

import torch

import _conv_classes as CC

P = 3
G31, G32 = 2 ** 31, 2 ** 32
LIMIT = 0xF0000000            # RS_BUFFER_BYTES_LIMIT (csrc/common.h): operands of the buffer-offset kernels must be smaller
PEAK_BYTES = 16 * 2 ** 30     # a test's peak device memory stays below this
LOUD = 1e4                    # what the padding columns of the sources hold
SENTINEL = {2: 0x7BCD, 4: 0x7F8BCDEF}   # the bit patterns of tests/test_conv_plan_gpu.py, per element size
ESZ = {CC.F16: 2, CC.F32: 4, CC.SPLIT: 4}

# ---------------------------------------------------------------- conv cases that go through ops.conv2d (ld = (ld0, ldy, ldres), `out=`)
# L: the layer at its full batch; C1: channels of a second source (dense, behind the C0 = Cin - C1 of x0); kernel: what must have run;
# sk: split-K expected; big: the operands the row is there for, each of which must lie in (2^31, LIMIT) bytes
ConvCase = namedtuple("ConvCase", "name L ld C1 kernel sk big")
_L = CC.Layer
CONV_CASES = [
    ConvCase("igemm2-f16", _L(CC.F16, CC.F16, 33, 128, 128, 64, 128, 1, 1, 1, True), (2048, 2048, 2048), 0, "CK_IGEMM2", False, "x y res"),
    ConvCase("igemm2-f32", _L(CC.F32, CC.F32, 33, 128, 128, 64, 128, 1, 1, 1, True), (1024, 1024, 1024), 0, "CK_IGEMM2", False, "x y res"),
    # igemm3 takes 224 .. 320 tiles of 256 pixels: 16 images of 64 x 64 reach 2^31 bytes only through the wide rows
    ConvCase("igemm3-f16", _L(CC.F16, CC.F16, 16, 64, 64, 1024, 128, 1, 1, 1, True), (16392, 16392, 16392), 0, "CK_IGEMM3", False, "x y res"),
    ConvCase("split-1x1", _L(CC.SPLIT, CC.SPLIT, 33, 128, 128, 64, 64, 1, 1, 1, True), (1024, 1024, 1024), 0, "CK_SPLIT", False, "x y res"),
    ConvCase("split-3x3s2", _L(CC.SPLIT, CC.SPLIT, 33, 128, 128, 64, 64, 3, 2, 1, True), (1024, 4096, 4096), 0, "CK_SPLIT", False, "x y res"),
    ConvCase("split-splitk", _L(CC.SPLIT, CC.SPLIT, 32, 16, 16, 320, 320, 3, 2, 1, True), (65544, 262152, 262152), 0, "CK_SPLIT", True, "x y res"),
    # the halo kernel's four-images-per-tile geometry with split-K (its slabs finished by the reduce kernel): 8 x 8 planes, wide rows
    ConvCase("halo-seg8-splitk", _L(CC.SPLIT, CC.SPLIT, 32, 8, 8, 640, 640, 3, 1, 1, True), (262152, 262152, 262152), 0, "CK_HALO_SEG", True, "x y res"),
    ConvCase("igemm-two-sources", _L(CC.F16, CC.F16, 33, 128, 128, 128, 64, 3, 1, 1, True), (2048, 64, 64), 64, "CK_IGEMM", False, "x"),
    # the two direct kernels (one thread per output element; one thread per pixel for Cout <= 8), fp32 results
    ConvCase("direct-f32", _L(CC.F16, CC.F32, 33, 128, 128, 3, 16, 3, 1, 1, False), (2048, 1024, 1024), 0, "CK_NONE", False, "x y"),
    ConvCase("direct-smallcout-f32", _L(CC.F16, CC.F32, 33, 128, 128, 8, 3, 3, 1, 1, False), (2048, 1024, 1024), 0, "CK_NONE", False, "x y"),
]
# Boundary of the buffer-offset families that ops.conv2d reaches: x0 alone is large (y and the residual dense), `per` bytes per image; the
# accepted batch is the largest below LIMIT, the refused one the next.  (ld0, B) make LIMIT a whole number of images, so the refused
# operand is exactly LIMIT bytes.
BOUNDARY_CONV = [
    ConvCase("igemm2-f16", _L(CC.F16, CC.F16, 59, 128, 128, 64, 128, 1, 1, 1, False), (2048, 128, 128), 0, "CK_IGEMM2", False, "x"),
    ConvCase("igemm3-f16", _L(CC.F16, CC.F16, 19, 64, 64, 1024, 128, 1, 1, 1, False), (24576, 128, 128), 0, "CK_IGEMM3", False, "x"),
    ConvCase("halo-f16", _L(CC.F16, CC.F16, 59, 128, 128, 64, 128, 3, 1, 1, False), (2048, 128, 128), 0, "CK_HALO", False, "x"),
    ConvCase("split-1x1", _L(CC.SPLIT, CC.SPLIT, 59, 128, 128, 64, 64, 1, 1, 1, False), (1024, 64, 64), 0, "CK_SPLIT", False, "x"),
]

# ---------------------------------------------------------------- cases of the dense wrappers: [B, H, W, C] NHWC, `esz` bytes per element
# (B, H, W, Cin, Cout, split) of ops.conv3x3_halo / ops.conv3x3_wino: input transform (coef + SiLU), statistics, residual
HALO_F16 = (513, 128, 128, 128, 128, False)
HALO_SPLIT = (257, 128, 128, 128, 128, True)
WINO_SPLIT = (513, 128, 128, 64, 64, True)
WINO_BOUNDARY = (959, 128, 128, 64, 64, True)      # 4 MiB per image: 960 images are LIMIT bytes
# (B, H, W) of the fused attention (E = 192, 6 heads): projection and shortcut
ATTN_F16 = (1366, 64, 64)
ATTN_SPLIT = (683, 64, 64)
ATTN_F16_BOUNDARY = (2559, 64, 64)                 # 1.5 MiB per image: 2560 images are LIMIT bytes
ATTN_SPLIT_BOUNDARY = (1279, 64, 64)               # 3 MiB per image
# fused Swin MLP: `B` blocks of 4096 tokens of 192 features (a block is the period's "image")
MLP_F16 = (1366, 4096)
MLP_SPLIT = (683, 4096)
# GroupNorm (statistics pass + apply pass: planes above 256 pixels) and the layout / storage kernels: more than 2^31 ELEMENTS
GN_SHAPE = (2049, 64, 64, 256)
ELEMENTWISE_SHAPE = (2049, 64, 64, 256)


def conv_bytes(c):
    """bytes per image of x0, y and the residual of a ConvCase, as the launch addresses them (the whole wide rows)"""
    L = c.L
    Ho, Wo = CC.out_hw(L)
    return {"x": L.H * L.W * c.ld[0] * ESZ[L.in_prec], "y": Ho * Wo * c.ld[1] * ESZ[L.out_prec], "res": Ho * Wo * c.ld[2] * ESZ[L.out_prec] if L.res else 0}


def dense_bytes(shape, C, esz):
    return shape[1] * shape[2] * C * esz


def dense_halo_plan(shape):
    """ops.conv_plan's answer for a dense (B, H, W, Cin, Cout, split) 3x3 layer with a residual, as ops.conv3x3_halo launches it"""
    from resshift_amd import ops

    B, H, W, Cin, Cout, split = shape
    return CC.Plan(*ops.conv_plan(B, H, W, Cin, Cout, 3, CC.SPLIT if split else CC.F16, has_res=True))


def alias_visible(bytes_per_image, period=P):
    """neither 2^31 nor 2^32 bytes is a whole number of periods: an address that is off by either reads other data"""
    return G31 % (period * bytes_per_image) != 0 and G32 % (period * bytes_per_image) != 0


def seed_of(*what):
    return zlib.crc32(repr(what).encode())


def conv_plan_of(c, dense=False):
    """ops.conv_plan's answer for a ConvCase (`dense`: the same layer without the wide rows)"""
    from resshift_amd import ops

    L = c.L
    p = ops.conv_plan(L.B, L.H, L.W, L.Cin - c.C1, L.Cout, L.k, L.in_prec, L.out_prec, C1=c.C1, stride=L.stride, up=L.up, has_res=L.res,
                      ld=None if dense else c.ld)
    return None if p is None else CC.Plan(*p)


# ---------------------------------------------------------------- device side
def free():
    gc.collect()
    torch.cuda.empty_cache()


def tile(base, B):
    """[P, ...] -> [B, ...]: the base images repeated with period P along the batch, materialised"""
    assert base.shape[0] == P
    return base.repeat((B + P - 1) // P, *([1] * (base.dim() - 1)))[:B]


def store(t_nchw, prec, dev, ld=None):
    """fp32 NCHW -> NHWC device tensor in storage `prec`, rows of `ld` elements whose columns behind the channels hold LOUD"""
    from resshift_amd import ops

    t = t_nchw.to(dev, torch.float32).permute(0, 2, 3, 1)
    C = t.shape[3]
    buf = torch.full((*t.shape[:3], C if ld is None else ld), LOUD, device=dev, dtype=torch.float32)
    buf[..., :C] = t
    return buf.half() if prec == CC.F16 else ops.convert(buf, ops.SPLIT) if prec == CC.SPLIT else buf


def load(y, prec, C):
    """stored NHWC [..., ld] -> fp32 NCHW of its first C columns"""
    from resshift_amd import ops

    y = ops.convert(y.contiguous(), ops.F32) if prec == CC.SPLIT else y
    return y[..., :C].permute(0, 3, 1, 2)


def sentinel_fill(t):
    esz = t.element_size()
    t.view(torch.int16 if esz == 2 else torch.int32).fill_(SENTINEL[esz])
    return t


def _bits(y):
    """integer view of a stored tensor whose last axis runs over its row's elements: [..., ld] (fp16, fp32) or [..., 2, ld] (split: hi | lo)"""
    if y.dtype == torch.int32:
        return y.view(torch.int16).view(*y.shape[:-1], 2, y.shape[-1])
    return y.view(torch.int16 if y.dtype == torch.float16 else torch.int32)


def sentinel_intact(t, first_col=0, chunk=4):
    """columns first_col .. of every row of t still hold the sentinel's bits (split storage: of both halves of the row)"""
    want = _bits(sentinel_fill(torch.empty_like(t[:1])))[..., first_col:]
    v = _bits(t)
    return all(bool((v[i:i + chunk][..., first_col:] == want).all()) for i in range(0, v.shape[0], chunk))


def rel_err_all_images(got_chunk, ref, B, chunk=2 * P):
    """max over ALL images b of |got[b] - ref[b % P]|, relative to max |ref|; got_chunk(b0, b1) -> images b0 .. b1 - 1 of the result in the
    reference's layout (any float type, on the reference's device); chunks start at multiples of P"""
    assert ref.shape[0] == P and chunk % P == 0 and ref.dtype == torch.float64
    scale = ref.abs().max().item() + 1e-12
    rep = ref.repeat(chunk // P, *([1] * (ref.dim() - 1)))
    worst = 0.0
    for b0 in range(0, B, chunk):
        b1 = min(B, b0 + chunk)
        got = got_chunk(b0, b1).to(torch.float64)
        assert got.shape == rep[:b1 - b0].shape, (got.shape, rep.shape)
        err = (got - rep[:b1 - b0]).abs().max().item()
        if not math.isfinite(err):
            return float("inf")
        worst = max(worst, err)
    return worst / scale


def equal_all_images(got_chunk, want_chunk, B, chunk=16):
    """got_chunk(b0, b1) and want_chunk(b0, b1) agree exactly, chunk by chunk"""
    return all(torch.equal(got_chunk(b0, min(B, b0 + chunk)), want_chunk(b0, min(B, b0 + chunk))) for b0 in range(0, B, chunk))


def stats_rel_err(st, y_chunk, B, chunk=2 * P):
    """the statistics slabs [B, slabs, C, 2] of a launch, summed over the slabs, against the sums and sums of squares of the stored result
    (y_chunk(b0, b1): its images as NCHW), as tests/test_ops_gpu.py compares them: max |got - want| / (|want| + 1)"""
    worst = 0.0
    for b0 in range(0, B, chunk):
        b1 = min(B, b0 + chunk)
        v = y_chunk(b0, b1).to(torch.float64).flatten(2)
        want = torch.stack([v.sum(-1), (v * v).sum(-1)], -1)
        got = st[b0:b1].to(torch.float64).sum(1)
        worst = max(worst, ((got - want).abs() / (want.abs() + 1.0)).max().item())
    return worst

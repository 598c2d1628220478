"""The conv planner's decision space as data: a grid of model-like layers, the class of a plan, and one committed representative per class.

rs_conv_plan (resshift_amd/csrc/igemm.hip) picks kernel, pixel tile, channel tile, small-plane segment, split-K factor and statistics slab per
launch.  `GRID` spans what the tile pool, the continuous sampler and out_scale can ask of it; `class_key` names what the planner decided;
`REPRESENTATIVES` holds the cheapest layer of every class with the plan expected of it, `EDGE_REPRESENTATIVES` the cheapest layer of every
(types, kernel, split-K yes/no, ragged M, ragged N, ragged K slice) combination.  tests/test_conv_plan_cpu.py pins both tables to the planner and
to the grid (closure: no class without a row); tests/test_conv_plan_gpu.py runs every row against float64.

After a planner change:  python tests/_conv_classes.py  prints the two tables anew (paste them over the literals below).
"""
import os
from collections import namedtuple

F16, F32, SPLIT = 0, 1, 2   # resshift_amd.ops.F16 / F32 / SPLIT

# ---- the grid -------------------------------------------------------------------------------------------------------------------------------
CIN = (64, 128, 160, 192, 256, 320, 384, 480, 512, 640, 768, 960, 1280)
COUT = (16, 48, 64, 128, 160, 192, 256, 320, 384, 480, 512, 640, 768, 960, 1280)
PLANES = ((8, 8), (8, 16), (16, 16), (24, 16), (16, 32), (32, 32), (32, 64), (64, 32), (60, 52), (64, 64), (64, 128), (128, 64), (96, 96), (128, 128))
BATCHES = tuple(range(1, 33))
MAX_PIXELS = 32 * 64 * 64           # of the output grid, B * Ho * Wo
OPS = ((1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 1, 2))   # (k, stride, up): 1x1, 3x3, 3x3 stride 2, 3x3 behind the folded nearest x2 upsample
STORAGE = ((F16, F16), (F16, F32), (F32, F32), (SPLIT, SPLIT), (SPLIT, F32))   # (in, out): the pairs rs_conv_plan documents
PLANNER_ENV = ("RS_IGEMM_", "RS_WINO", "RS_SPLIT", "RS_SPLITK_")   # the planner reads these once per process

Layer = namedtuple("Layer", "in_prec out_prec B H W Cin Cout k stride up res")
Plan = namedtuple("Plan", "kernel BP BC SEG splitk stats_px")


def planner_env():
    """the planner knobs set in this process's environment (the tables hold for none)"""
    return sorted(k for k in os.environ if k.startswith(PLANNER_ENV))


def out_hw(L):
    pad = L.k // 2
    return (L.H * L.up + 2 * pad - L.k) // L.stride + 1, (L.W * L.up + 2 * pad - L.k) // L.stride + 1


def grid_blocks():
    """the grid without its channel and residual axes, in the grid's order (Cin, Cout and res of the layers yielded are placeholders)"""
    for in_prec, out_prec in STORAGE:
        for k, stride, up in OPS:
            for H, W in PLANES:
                Ho, Wo = out_hw(Layer(in_prec, out_prec, 1, H, W, 0, 0, k, stride, up, False))
                for B in BATCHES:
                    if B * Ho * Wo <= MAX_PIXELS:
                        yield Layer(in_prec, out_prec, B, H, W, 0, 0, k, stride, up, False)


def grid_sample(n, seed=0):
    """n layers drawn evenly from the whole grid (every axis, the residual included)"""
    import random

    rnd, blocks = random.Random(seed), list(grid_blocks())
    return [rnd.choice(blocks)._replace(Cin=rnd.choice(CIN), Cout=rnd.choice(COUT), res=rnd.random() < 0.5) for _ in range(n)]


def plan_of(L, ld=None):
    """ops.conv_plan's answer for a layer, as a Plan (None: no kernel takes it)"""
    from resshift_amd import ops

    p = ops.conv_plan(L.B, L.H, L.W, L.Cin, L.Cout, L.k, L.in_prec, L.out_prec, stride=L.stride, up=L.up, has_res=L.res, ld=ld)
    return None if p is None else Plan(*p)


def gemm_dims(L):
    Ho, Wo = out_hw(L)
    return L.B * Ho * Wo, L.k * L.k * L.Cin, L.Cout   # M, K, N


def cost(L):
    M, K, N = gemm_dims(L)
    return M * K * N


def splitk_bucket(sk):
    return "1" if sk <= 1 else "2" if sk == 2 else "3-4" if sk <= 4 else "5-8" if sk <= 8 else "9-16" if sk <= 16 else ">16"


def class_key(L, p):
    """(in type, out type, kernel, BP, BC, SEG, split-K bucket, statistics yes / no)"""
    return (L.in_prec, L.out_prec, p.kernel, p.BP, p.BC, p.SEG, splitk_bucket(p.splitk), p.stats_px > 0)


def k_stages(L):
    """K stages of a launch: 64 halfs of K per stage, 32 floats in fp32 storage (igemm.hip, igemm_split.hip)"""
    bk = 32 if L.in_prec == F32 else 64
    return (gemm_dims(L)[1] + bk - 1) // bk


def edge_key(L, p):
    """(in type, out type, kernel, split-K yes / no, ragged M, ragged N, ragged K slice)"""
    M, _, N = gemm_dims(L)
    return (L.in_prec, L.out_prec, p.kernel, p.splitk > 1, M % p.BP != 0, N % p.BC != 0, p.splitk > 1 and k_stages(L) % p.splitk != 0)


def classes_of_grid():
    """({class key: (layer, plan)}, {edge key: (layer, plan)}) with the layer of smallest M*K*Cout per key, ties broken by the grid's order"""
    import ctypes

    from resshift_amd import _lib, ops

    # millions of layers: the planner is asked through the C entry itself and the keys are first formed from its raw integers, per kernel size
    # (one cost scale per key); `ops.conv_plan`, `class_key` and `edge_key` then name the winners and merge the kernel sizes
    query, out = _lib.load().rs_op_conv_plan, (ctypes.c_int * 6)()
    best, edge = {}, {}
    for L in grid_blocks():
        (Ho, Wo), pad = out_hw(L), L.k // 2
        M, stages = L.B * Ho * Wo, [(L.k * L.k * cin + (31 if L.in_prec == F32 else 63)) // (32 if L.in_prec == F32 else 64) for cin in CIN]
        for cin, nk in zip(CIN, stages):
            for cout in COUT:
                for res in (0, 1):
                    rc = query(L.B, L.H, L.W, cin, 0, cout, L.k, L.k, L.stride, pad, pad, Ho, Wo, L.up, 0, L.in_prec, L.out_prec, cin, 0, cout,
                               cout, res, 1, out)
                    kern, BP, BC, SEG, sk, spx = out
                    if rc or not kern:
                        raise AssertionError(f"no kernel takes {L._replace(Cin=cin, Cout=cout, res=bool(res))}")
                    c = M * cin * cout   # (k is one per block: M * K * Cout up to that factor)
                    ck = (L.in_prec, L.out_prec, L.k, kern, BP, BC, SEG, sk if sk < 3 else (sk + 3) // 4 * 4 if sk <= 8 else 16 if sk <= 16 else 17, spx > 0)
                    ek = (L.in_prec, L.out_prec, L.k, kern, sk > 1, M % BP != 0, cout % BC != 0, sk > 1 and nk % sk != 0)
                    for table, key in ((best, ck), (edge, ek)):
                        if key not in table or c < table[key][0]:
                            table[key] = (c, L.B, L.H, L.W, cin, cout, L.stride, L.up, res)
    result = []
    for table, keyfn in ((best, class_key), (edge, edge_key)):
        named = {}
        for (in_prec, out_prec, k, *_), (_, B, H, W, cin, cout, stride, up, res) in table.items():   # (dicts keep the grid's order)
            L = Layer(in_prec, out_prec, B, H, W, cin, cout, k, stride, up, bool(res))
            p = plan_of(L)
            key = keyfn(L, p)
            if key not in named or cost(L) < cost(named[key][0]):
                named[key] = (L, p)
        result.append(named)
    return tuple(result)


def regenerate():
    """the text of the two literal tables below, from the planner as it is now"""
    best, edge = classes_of_grid()
    out = []
    for name, table in (("REPRESENTATIVES", best), ("EDGE_REPRESENTATIVES", edge)):
        out.append(f"{name} = [")
        for key in sorted(table):
            L, p = table[key]
            out.append(f"    ({tuple(L)!r}, {tuple(p)!r}),")
        out.append("]")
    return "\n".join(out)


def rows(table):
    return [(Layer(*L), Plan(*p)) for L, p in table]


def row_id(L, p):
    prec = {F16: "h", F32: "f", SPLIT: "s"}
    return (f"{prec[L.in_prec]}{prec[L.out_prec]}-{p.kernel[3:].lower()}-{p.BP}x{p.BC}-sk{p.splitk}-"
            f"{L.B}x{L.H}x{L.W}-{L.Cin}to{L.Cout}-k{L.k}s{L.stride}u{L.up}{'r' if L.res else ''}")


# ---- the committed tables: (layer, expected plan) -----------------------------------------------------------------------------------------------
# layer = (in_prec, out_prec, B, H, W, Cin, Cout, k, stride, up, res); plan = (kernel, BP, BC, SEG, splitk, stats_px)
# TABLES-BEGIN
REPRESENTATIVES = [
    ((0, 0, 16, 16, 32, 64, 768, 3, 1, 1, False), ('CK_HALO', 32, 128, 0, 1, 256)),
    ((0, 0, 16, 16, 32, 64, 960, 3, 1, 1, False), ('CK_HALO', 32, 160, 0, 1, 256)),
    ((0, 0, 24, 64, 32, 64, 192, 3, 1, 1, False), ('CK_HALO', 32, 192, 0, 1, 256)),
    ((0, 0, 4, 32, 64, 64, 768, 3, 1, 1, False), ('CK_HALO', 64, 128, 0, 1, 256)),
    ((0, 0, 24, 32, 64, 64, 192, 3, 1, 1, False), ('CK_HALO', 64, 192, 0, 1, 256)),
    ((0, 0, 1, 8, 8, 64, 16, 1, 1, 1, False), ('CK_IGEMM', 64, 64, 0, 1, 0)),
    ((0, 0, 1, 8, 8, 128, 16, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 2, 0)),
    ((0, 0, 1, 8, 8, 192, 16, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 3, 0)),
    ((0, 0, 1, 8, 8, 320, 16, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 5, 0)),
    ((0, 0, 1, 8, 8, 512, 16, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 9, 0)),
    ((0, 0, 1, 60, 52, 64, 16, 1, 1, 1, False), ('CK_IGEMM', 128, 64, 0, 1, 0)),
    ((0, 0, 1, 60, 52, 128, 16, 3, 1, 1, False), ('CK_IGEMM', 128, 64, 0, 2, 0)),
    ((0, 0, 1, 60, 52, 192, 16, 3, 1, 1, False), ('CK_IGEMM', 128, 64, 0, 3, 0)),
    ((0, 0, 1, 60, 52, 320, 16, 3, 1, 1, False), ('CK_IGEMM', 128, 64, 0, 5, 0)),
    ((0, 0, 1, 60, 52, 512, 16, 3, 1, 1, False), ('CK_IGEMM', 128, 64, 0, 9, 0)),
    ((0, 0, 1, 8, 8, 64, 128, 1, 1, 1, False), ('CK_IGEMM2', 64, 128, 0, 1, 0)),
    ((0, 0, 1, 8, 8, 128, 128, 3, 2, 1, False), ('CK_IGEMM2', 64, 128, 0, 2, 0)),
    ((0, 0, 1, 8, 8, 192, 128, 3, 2, 1, False), ('CK_IGEMM2', 64, 128, 0, 3, 0)),
    ((0, 0, 1, 8, 8, 320, 128, 3, 2, 1, False), ('CK_IGEMM2', 64, 128, 0, 5, 0)),
    ((0, 0, 1, 8, 8, 512, 128, 3, 2, 1, False), ('CK_IGEMM2', 64, 128, 0, 9, 0)),
    ((0, 0, 1, 8, 8, 64, 160, 1, 1, 1, False), ('CK_IGEMM2', 64, 160, 0, 1, 0)),
    ((0, 0, 1, 8, 8, 128, 160, 3, 2, 1, False), ('CK_IGEMM2', 64, 160, 0, 2, 0)),
    ((0, 0, 1, 8, 8, 192, 160, 3, 2, 1, False), ('CK_IGEMM2', 64, 160, 0, 3, 0)),
    ((0, 0, 1, 8, 8, 320, 160, 3, 2, 1, False), ('CK_IGEMM2', 64, 160, 0, 5, 0)),
    ((0, 0, 1, 8, 8, 512, 160, 3, 2, 1, False), ('CK_IGEMM2', 64, 160, 0, 9, 0)),
    ((0, 0, 1, 8, 8, 64, 192, 1, 1, 1, False), ('CK_IGEMM2', 64, 192, 0, 1, 0)),
    ((0, 0, 1, 8, 8, 128, 192, 3, 2, 1, False), ('CK_IGEMM2', 64, 192, 0, 2, 0)),
    ((0, 0, 1, 8, 8, 192, 192, 3, 2, 1, False), ('CK_IGEMM2', 64, 192, 0, 3, 0)),
    ((0, 0, 1, 8, 8, 320, 192, 3, 2, 1, False), ('CK_IGEMM2', 64, 192, 0, 5, 0)),
    ((0, 0, 1, 8, 8, 512, 192, 3, 2, 1, False), ('CK_IGEMM2', 64, 192, 0, 9, 0)),
    ((0, 0, 22, 24, 16, 64, 128, 1, 1, 1, False), ('CK_IGEMM2', 128, 128, 0, 1, 0)),
    ((0, 0, 22, 24, 16, 128, 128, 3, 1, 1, False), ('CK_IGEMM2', 128, 128, 0, 2, 0)),
    ((0, 0, 22, 24, 16, 192, 128, 3, 1, 1, False), ('CK_IGEMM2', 128, 128, 0, 3, 0)),
    ((0, 0, 22, 24, 16, 320, 128, 3, 1, 1, False), ('CK_IGEMM2', 128, 128, 0, 5, 0)),
    ((0, 0, 22, 24, 16, 64, 160, 1, 1, 1, False), ('CK_IGEMM2', 128, 160, 0, 1, 0)),
    ((0, 0, 22, 24, 16, 128, 160, 3, 1, 1, False), ('CK_IGEMM2', 128, 160, 0, 2, 0)),
    ((0, 0, 22, 24, 16, 192, 160, 3, 1, 1, False), ('CK_IGEMM2', 128, 160, 0, 3, 0)),
    ((0, 0, 22, 24, 16, 320, 160, 3, 1, 1, False), ('CK_IGEMM2', 128, 160, 0, 5, 0)),
    ((0, 0, 22, 24, 16, 64, 192, 1, 1, 1, False), ('CK_IGEMM2', 128, 192, 0, 1, 0)),
    ((0, 0, 22, 24, 16, 128, 192, 3, 1, 1, False), ('CK_IGEMM2', 128, 192, 0, 2, 0)),
    ((0, 0, 22, 24, 16, 192, 192, 3, 1, 1, False), ('CK_IGEMM2', 128, 192, 0, 3, 0)),
    ((0, 0, 22, 24, 16, 320, 192, 3, 1, 1, False), ('CK_IGEMM2', 128, 192, 0, 5, 0)),
    ((0, 0, 28, 32, 64, 128, 512, 3, 2, 1, False), ('CK_IGEMM3', 256, 128, 0, 1, 0)),
    ((0, 0, 9, 60, 52, 128, 1280, 3, 2, 1, False), ('CK_IGEMM3', 256, 160, 0, 1, 0)),
    ((0, 1, 1, 8, 8, 64, 16, 1, 1, 1, False), ('CK_IGEMM', 64, 64, 0, 1, 0)),
    ((0, 1, 1, 8, 8, 128, 16, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 2, 0)),
    ((0, 1, 1, 8, 8, 192, 16, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 3, 0)),
    ((0, 1, 1, 8, 8, 320, 16, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 5, 0)),
    ((0, 1, 1, 8, 8, 512, 16, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 9, 0)),
    ((0, 1, 1, 60, 52, 64, 16, 1, 1, 1, False), ('CK_IGEMM', 128, 64, 0, 1, 0)),
    ((0, 1, 1, 60, 52, 128, 16, 3, 1, 1, False), ('CK_IGEMM', 128, 64, 0, 2, 0)),
    ((0, 1, 1, 60, 52, 192, 16, 3, 1, 1, False), ('CK_IGEMM', 128, 64, 0, 3, 0)),
    ((0, 1, 1, 60, 52, 320, 16, 3, 1, 1, False), ('CK_IGEMM', 128, 64, 0, 5, 0)),
    ((0, 1, 1, 60, 52, 512, 16, 3, 1, 1, False), ('CK_IGEMM', 128, 64, 0, 9, 0)),
    ((0, 1, 1, 8, 8, 64, 128, 1, 1, 1, False), ('CK_IGEMM2', 64, 128, 0, 1, 0)),
    ((0, 1, 1, 8, 8, 128, 128, 3, 2, 1, False), ('CK_IGEMM2', 64, 128, 0, 2, 0)),
    ((0, 1, 1, 8, 8, 192, 128, 3, 2, 1, False), ('CK_IGEMM2', 64, 128, 0, 3, 0)),
    ((0, 1, 1, 8, 8, 320, 128, 3, 2, 1, False), ('CK_IGEMM2', 64, 128, 0, 5, 0)),
    ((0, 1, 1, 8, 8, 512, 128, 3, 2, 1, False), ('CK_IGEMM2', 64, 128, 0, 9, 0)),
    ((0, 1, 1, 8, 8, 64, 160, 1, 1, 1, False), ('CK_IGEMM2', 64, 160, 0, 1, 0)),
    ((0, 1, 1, 8, 8, 128, 160, 3, 2, 1, False), ('CK_IGEMM2', 64, 160, 0, 2, 0)),
    ((0, 1, 1, 8, 8, 192, 160, 3, 2, 1, False), ('CK_IGEMM2', 64, 160, 0, 3, 0)),
    ((0, 1, 1, 8, 8, 320, 160, 3, 2, 1, False), ('CK_IGEMM2', 64, 160, 0, 5, 0)),
    ((0, 1, 1, 8, 8, 512, 160, 3, 2, 1, False), ('CK_IGEMM2', 64, 160, 0, 9, 0)),
    ((0, 1, 1, 8, 8, 64, 192, 1, 1, 1, False), ('CK_IGEMM2', 64, 192, 0, 1, 0)),
    ((0, 1, 1, 8, 8, 128, 192, 3, 2, 1, False), ('CK_IGEMM2', 64, 192, 0, 2, 0)),
    ((0, 1, 1, 8, 8, 192, 192, 3, 2, 1, False), ('CK_IGEMM2', 64, 192, 0, 3, 0)),
    ((0, 1, 1, 8, 8, 320, 192, 3, 2, 1, False), ('CK_IGEMM2', 64, 192, 0, 5, 0)),
    ((0, 1, 1, 8, 8, 512, 192, 3, 2, 1, False), ('CK_IGEMM2', 64, 192, 0, 9, 0)),
    ((0, 1, 22, 24, 16, 64, 128, 1, 1, 1, False), ('CK_IGEMM2', 128, 128, 0, 1, 0)),
    ((0, 1, 22, 24, 16, 128, 128, 3, 1, 1, False), ('CK_IGEMM2', 128, 128, 0, 2, 0)),
    ((0, 1, 22, 24, 16, 192, 128, 3, 1, 1, False), ('CK_IGEMM2', 128, 128, 0, 3, 0)),
    ((0, 1, 22, 24, 16, 320, 128, 3, 1, 1, False), ('CK_IGEMM2', 128, 128, 0, 5, 0)),
    ((0, 1, 22, 24, 16, 64, 160, 1, 1, 1, False), ('CK_IGEMM2', 128, 160, 0, 1, 0)),
    ((0, 1, 22, 24, 16, 128, 160, 3, 1, 1, False), ('CK_IGEMM2', 128, 160, 0, 2, 0)),
    ((0, 1, 22, 24, 16, 192, 160, 3, 1, 1, False), ('CK_IGEMM2', 128, 160, 0, 3, 0)),
    ((0, 1, 22, 24, 16, 320, 160, 3, 1, 1, False), ('CK_IGEMM2', 128, 160, 0, 5, 0)),
    ((0, 1, 22, 24, 16, 64, 192, 1, 1, 1, False), ('CK_IGEMM2', 128, 192, 0, 1, 0)),
    ((0, 1, 22, 24, 16, 128, 192, 3, 1, 1, False), ('CK_IGEMM2', 128, 192, 0, 2, 0)),
    ((0, 1, 22, 24, 16, 192, 192, 3, 1, 1, False), ('CK_IGEMM2', 128, 192, 0, 3, 0)),
    ((0, 1, 22, 24, 16, 320, 192, 3, 1, 1, False), ('CK_IGEMM2', 128, 192, 0, 5, 0)),
    ((0, 1, 28, 16, 32, 128, 512, 3, 1, 1, False), ('CK_IGEMM3', 256, 128, 0, 1, 0)),
    ((0, 1, 9, 60, 52, 128, 1280, 3, 2, 1, False), ('CK_IGEMM3', 256, 160, 0, 1, 0)),
    ((1, 1, 1, 8, 8, 64, 16, 1, 1, 1, False), ('CK_IGEMM', 64, 64, 0, 1, 0)),
    ((1, 1, 1, 8, 8, 64, 16, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 2, 0)),
    ((1, 1, 1, 8, 8, 128, 16, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 4, 0)),
    ((1, 1, 1, 8, 8, 160, 16, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 5, 0)),
    ((1, 1, 1, 8, 8, 256, 16, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 9, 0)),
    ((1, 1, 1, 60, 52, 64, 16, 1, 1, 1, False), ('CK_IGEMM', 128, 64, 0, 1, 0)),
    ((1, 1, 1, 60, 52, 512, 16, 1, 1, 1, False), ('CK_IGEMM', 128, 64, 0, 2, 0)),
    ((1, 1, 1, 60, 52, 768, 16, 1, 1, 1, False), ('CK_IGEMM', 128, 64, 0, 3, 0)),
    ((1, 1, 1, 60, 52, 1280, 16, 1, 1, 1, False), ('CK_IGEMM', 128, 64, 0, 5, 0)),
    ((1, 1, 1, 60, 52, 256, 16, 3, 1, 1, False), ('CK_IGEMM', 128, 64, 0, 9, 0)),
    ((1, 1, 1, 8, 8, 64, 128, 1, 1, 1, False), ('CK_IGEMM2', 64, 128, 0, 1, 0)),
    ((1, 1, 1, 8, 8, 64, 128, 3, 2, 1, False), ('CK_IGEMM2', 64, 128, 0, 2, 0)),
    ((1, 1, 1, 8, 8, 128, 128, 3, 2, 1, False), ('CK_IGEMM2', 64, 128, 0, 4, 0)),
    ((1, 1, 1, 8, 8, 160, 128, 3, 2, 1, False), ('CK_IGEMM2', 64, 128, 0, 5, 0)),
    ((1, 1, 1, 8, 8, 256, 128, 3, 2, 1, False), ('CK_IGEMM2', 64, 128, 0, 9, 0)),
    ((1, 1, 1, 8, 8, 64, 160, 1, 1, 1, False), ('CK_IGEMM2', 64, 160, 0, 1, 0)),
    ((1, 1, 1, 8, 8, 64, 160, 3, 2, 1, False), ('CK_IGEMM2', 64, 160, 0, 2, 0)),
    ((1, 1, 1, 8, 8, 128, 160, 3, 2, 1, False), ('CK_IGEMM2', 64, 160, 0, 4, 0)),
    ((1, 1, 1, 8, 8, 160, 160, 3, 2, 1, False), ('CK_IGEMM2', 64, 160, 0, 5, 0)),
    ((1, 1, 1, 8, 8, 256, 160, 3, 2, 1, False), ('CK_IGEMM2', 64, 160, 0, 9, 0)),
    ((1, 1, 1, 8, 8, 64, 192, 1, 1, 1, False), ('CK_IGEMM2', 64, 192, 0, 1, 0)),
    ((1, 1, 1, 8, 8, 64, 192, 3, 2, 1, False), ('CK_IGEMM2', 64, 192, 0, 2, 0)),
    ((1, 1, 1, 8, 8, 128, 192, 3, 2, 1, False), ('CK_IGEMM2', 64, 192, 0, 4, 0)),
    ((1, 1, 1, 8, 8, 160, 192, 3, 2, 1, False), ('CK_IGEMM2', 64, 192, 0, 5, 0)),
    ((1, 1, 1, 8, 8, 256, 192, 3, 2, 1, False), ('CK_IGEMM2', 64, 192, 0, 9, 0)),
    ((1, 1, 22, 24, 16, 64, 128, 1, 1, 1, False), ('CK_IGEMM2', 128, 128, 0, 1, 0)),
    ((1, 1, 22, 24, 16, 512, 128, 1, 1, 1, False), ('CK_IGEMM2', 128, 128, 0, 2, 0)),
    ((1, 1, 22, 24, 16, 768, 128, 1, 1, 1, False), ('CK_IGEMM2', 128, 128, 0, 3, 0)),
    ((1, 1, 22, 24, 16, 1280, 128, 1, 1, 1, False), ('CK_IGEMM2', 128, 128, 0, 5, 0)),
    ((1, 1, 22, 24, 16, 64, 160, 1, 1, 1, False), ('CK_IGEMM2', 128, 160, 0, 1, 0)),
    ((1, 1, 22, 24, 16, 512, 160, 1, 1, 1, False), ('CK_IGEMM2', 128, 160, 0, 2, 0)),
    ((1, 1, 22, 24, 16, 768, 160, 1, 1, 1, False), ('CK_IGEMM2', 128, 160, 0, 3, 0)),
    ((1, 1, 22, 24, 16, 1280, 160, 1, 1, 1, False), ('CK_IGEMM2', 128, 160, 0, 5, 0)),
    ((1, 1, 22, 24, 16, 64, 192, 1, 1, 1, False), ('CK_IGEMM2', 128, 192, 0, 1, 0)),
    ((1, 1, 22, 24, 16, 512, 192, 1, 1, 1, False), ('CK_IGEMM2', 128, 192, 0, 2, 0)),
    ((1, 1, 22, 24, 16, 768, 192, 1, 1, 1, False), ('CK_IGEMM2', 128, 192, 0, 3, 0)),
    ((1, 1, 22, 24, 16, 1280, 192, 1, 1, 1, False), ('CK_IGEMM2', 128, 192, 0, 5, 0)),
    ((2, 1, 1, 8, 8, 64, 16, 1, 1, 1, False), ('CK_SPLIT', 64, 64, 0, 1, 0)),
    ((2, 1, 1, 8, 8, 128, 16, 3, 2, 1, False), ('CK_SPLIT', 64, 64, 0, 2, 0)),
    ((2, 1, 1, 8, 8, 192, 16, 3, 2, 1, False), ('CK_SPLIT', 64, 64, 0, 3, 0)),
    ((2, 1, 1, 8, 8, 320, 16, 3, 2, 1, False), ('CK_SPLIT', 64, 64, 0, 5, 0)),
    ((2, 1, 1, 8, 8, 512, 16, 3, 2, 1, False), ('CK_SPLIT', 64, 64, 0, 9, 0)),
    ((2, 1, 1, 8, 8, 64, 128, 1, 1, 1, False), ('CK_SPLIT', 64, 128, 0, 1, 0)),
    ((2, 1, 1, 8, 8, 128, 128, 3, 2, 1, False), ('CK_SPLIT', 64, 128, 0, 2, 0)),
    ((2, 1, 1, 8, 8, 192, 128, 3, 2, 1, False), ('CK_SPLIT', 64, 128, 0, 3, 0)),
    ((2, 1, 1, 8, 8, 320, 128, 3, 2, 1, False), ('CK_SPLIT', 64, 128, 0, 5, 0)),
    ((2, 1, 1, 8, 8, 512, 128, 3, 2, 1, False), ('CK_SPLIT', 64, 128, 0, 9, 0)),
    ((2, 1, 1, 8, 8, 64, 160, 1, 1, 1, False), ('CK_SPLIT', 64, 160, 0, 1, 0)),
    ((2, 1, 1, 8, 8, 128, 160, 3, 2, 1, False), ('CK_SPLIT', 64, 160, 0, 2, 0)),
    ((2, 1, 1, 8, 8, 192, 160, 3, 2, 1, False), ('CK_SPLIT', 64, 160, 0, 3, 0)),
    ((2, 1, 1, 8, 8, 320, 160, 3, 2, 1, False), ('CK_SPLIT', 64, 160, 0, 5, 0)),
    ((2, 1, 1, 8, 8, 512, 160, 3, 2, 1, False), ('CK_SPLIT', 64, 160, 0, 9, 0)),
    ((2, 1, 1, 8, 8, 64, 192, 1, 1, 1, False), ('CK_SPLIT', 64, 192, 0, 1, 0)),
    ((2, 1, 1, 8, 8, 128, 192, 3, 2, 1, False), ('CK_SPLIT', 64, 192, 0, 2, 0)),
    ((2, 1, 1, 8, 8, 192, 192, 3, 2, 1, False), ('CK_SPLIT', 64, 192, 0, 3, 0)),
    ((2, 1, 1, 8, 8, 320, 192, 3, 2, 1, False), ('CK_SPLIT', 64, 192, 0, 5, 0)),
    ((2, 1, 1, 8, 8, 512, 192, 3, 2, 1, False), ('CK_SPLIT', 64, 192, 0, 9, 0)),
    ((2, 1, 32, 16, 16, 64, 16, 1, 1, 1, False), ('CK_SPLIT', 128, 64, 0, 1, 0)),
    ((2, 1, 32, 16, 16, 128, 16, 3, 1, 1, False), ('CK_SPLIT', 128, 64, 0, 2, 0)),
    ((2, 1, 32, 16, 16, 192, 16, 3, 1, 1, False), ('CK_SPLIT', 128, 64, 0, 3, 0)),
    ((2, 1, 31, 8, 8, 64, 512, 1, 1, 1, False), ('CK_SPLIT', 128, 128, 0, 1, 0)),
    ((2, 1, 1, 60, 52, 128, 1280, 3, 2, 1, False), ('CK_SPLIT', 128, 128, 0, 2, 0)),
    ((2, 1, 1, 60, 52, 192, 1280, 3, 2, 1, False), ('CK_SPLIT', 128, 128, 0, 3, 0)),
    ((2, 1, 21, 8, 8, 64, 960, 1, 1, 1, False), ('CK_SPLIT', 128, 160, 0, 1, 0)),
    ((2, 1, 21, 8, 8, 128, 960, 3, 1, 1, False), ('CK_SPLIT', 128, 160, 0, 2, 0)),
    ((2, 1, 21, 8, 8, 192, 960, 3, 1, 1, False), ('CK_SPLIT', 128, 160, 0, 3, 0)),
    ((2, 1, 32, 16, 16, 64, 192, 1, 1, 1, False), ('CK_SPLIT', 128, 192, 0, 1, 0)),
    ((2, 1, 32, 16, 16, 128, 192, 3, 1, 1, False), ('CK_SPLIT', 128, 192, 0, 2, 0)),
    ((2, 1, 32, 16, 16, 192, 192, 3, 1, 1, False), ('CK_SPLIT', 128, 192, 0, 3, 0)),
    ((2, 2, 16, 16, 32, 64, 768, 3, 1, 1, False), ('CK_HALO', 32, 128, 0, 1, 256)),
    ((2, 2, 16, 16, 32, 64, 960, 3, 1, 1, False), ('CK_HALO', 32, 160, 0, 1, 256)),
    ((2, 2, 4, 32, 64, 64, 768, 3, 1, 1, False), ('CK_HALO', 64, 128, 0, 1, 256)),
    ((2, 2, 4, 8, 8, 64, 128, 3, 1, 1, False), ('CK_HALO_SEG', 32, 128, 8, 3, 64)),
    ((2, 2, 4, 8, 8, 128, 128, 3, 1, 1, False), ('CK_HALO_SEG', 32, 128, 8, 6, 64)),
    ((2, 2, 4, 8, 8, 192, 128, 3, 1, 1, False), ('CK_HALO_SEG', 32, 128, 8, 9, 64)),
    ((2, 2, 4, 8, 8, 384, 128, 3, 1, 1, False), ('CK_HALO_SEG', 32, 128, 8, 18, 64)),
    ((2, 2, 4, 8, 8, 64, 160, 3, 1, 1, False), ('CK_HALO_SEG', 32, 160, 8, 3, 64)),
    ((2, 2, 4, 8, 8, 128, 160, 3, 1, 1, False), ('CK_HALO_SEG', 32, 160, 8, 6, 64)),
    ((2, 2, 4, 8, 8, 192, 160, 3, 1, 1, False), ('CK_HALO_SEG', 32, 160, 8, 9, 64)),
    ((2, 2, 4, 8, 8, 384, 160, 3, 1, 1, False), ('CK_HALO_SEG', 32, 160, 8, 18, 64)),
    ((2, 2, 1, 8, 8, 64, 16, 3, 2, 1, False), ('CK_SPLIT', 64, 64, 0, 1, 0)),
    ((2, 2, 1, 8, 8, 64, 16, 1, 1, 1, False), ('CK_SPLIT', 64, 64, 0, 1, 64)),
    ((2, 2, 1, 24, 16, 128, 16, 3, 1, 1, False), ('CK_SPLIT', 64, 64, 0, 2, 0)),
    ((2, 2, 1, 8, 8, 128, 16, 3, 2, 1, False), ('CK_SPLIT', 64, 64, 0, 2, 16)),
    ((2, 2, 1, 24, 16, 192, 16, 3, 1, 1, False), ('CK_SPLIT', 64, 64, 0, 3, 0)),
    ((2, 2, 1, 8, 8, 192, 16, 3, 2, 1, False), ('CK_SPLIT', 64, 64, 0, 3, 16)),
    ((2, 2, 1, 24, 16, 320, 16, 3, 1, 1, False), ('CK_SPLIT', 64, 64, 0, 5, 0)),
    ((2, 2, 1, 8, 8, 320, 16, 3, 2, 1, False), ('CK_SPLIT', 64, 64, 0, 5, 16)),
    ((2, 2, 1, 24, 16, 512, 16, 3, 1, 1, False), ('CK_SPLIT', 64, 64, 0, 9, 0)),
    ((2, 2, 1, 8, 8, 512, 16, 3, 2, 1, False), ('CK_SPLIT', 64, 64, 0, 9, 16)),
    ((2, 2, 1, 8, 8, 64, 128, 3, 2, 1, False), ('CK_SPLIT', 64, 128, 0, 1, 0)),
    ((2, 2, 1, 8, 8, 64, 128, 1, 1, 1, False), ('CK_SPLIT', 64, 128, 0, 1, 64)),
    ((2, 2, 1, 24, 16, 128, 128, 3, 1, 1, False), ('CK_SPLIT', 64, 128, 0, 2, 0)),
    ((2, 2, 1, 8, 8, 128, 128, 3, 2, 1, False), ('CK_SPLIT', 64, 128, 0, 2, 16)),
    ((2, 2, 1, 24, 16, 192, 128, 3, 1, 1, False), ('CK_SPLIT', 64, 128, 0, 3, 0)),
    ((2, 2, 1, 8, 8, 192, 128, 3, 2, 1, False), ('CK_SPLIT', 64, 128, 0, 3, 16)),
    ((2, 2, 1, 24, 16, 320, 128, 3, 1, 1, False), ('CK_SPLIT', 64, 128, 0, 5, 0)),
    ((2, 2, 1, 8, 8, 320, 128, 3, 2, 1, False), ('CK_SPLIT', 64, 128, 0, 5, 16)),
    ((2, 2, 1, 24, 16, 512, 128, 3, 1, 1, False), ('CK_SPLIT', 64, 128, 0, 9, 0)),
    ((2, 2, 1, 8, 8, 512, 128, 3, 2, 1, False), ('CK_SPLIT', 64, 128, 0, 9, 16)),
    ((2, 2, 1, 8, 8, 64, 160, 3, 2, 1, False), ('CK_SPLIT', 64, 160, 0, 1, 0)),
    ((2, 2, 1, 8, 8, 64, 160, 1, 1, 1, False), ('CK_SPLIT', 64, 160, 0, 1, 64)),
    ((2, 2, 1, 24, 16, 128, 160, 3, 1, 1, False), ('CK_SPLIT', 64, 160, 0, 2, 0)),
    ((2, 2, 1, 8, 8, 128, 160, 3, 2, 1, False), ('CK_SPLIT', 64, 160, 0, 2, 16)),
    ((2, 2, 1, 24, 16, 192, 160, 3, 1, 1, False), ('CK_SPLIT', 64, 160, 0, 3, 0)),
    ((2, 2, 1, 8, 8, 192, 160, 3, 2, 1, False), ('CK_SPLIT', 64, 160, 0, 3, 16)),
    ((2, 2, 1, 24, 16, 320, 160, 3, 1, 1, False), ('CK_SPLIT', 64, 160, 0, 5, 0)),
    ((2, 2, 1, 8, 8, 320, 160, 3, 2, 1, False), ('CK_SPLIT', 64, 160, 0, 5, 16)),
    ((2, 2, 1, 24, 16, 512, 160, 3, 1, 1, False), ('CK_SPLIT', 64, 160, 0, 9, 0)),
    ((2, 2, 1, 8, 8, 512, 160, 3, 2, 1, False), ('CK_SPLIT', 64, 160, 0, 9, 16)),
    ((2, 2, 1, 8, 8, 64, 192, 3, 2, 1, False), ('CK_SPLIT', 64, 192, 0, 1, 0)),
    ((2, 2, 1, 8, 8, 64, 192, 1, 1, 1, False), ('CK_SPLIT', 64, 192, 0, 1, 64)),
    ((2, 2, 1, 24, 16, 128, 192, 3, 1, 1, False), ('CK_SPLIT', 64, 192, 0, 2, 0)),
    ((2, 2, 1, 8, 8, 128, 192, 3, 2, 1, False), ('CK_SPLIT', 64, 192, 0, 2, 16)),
    ((2, 2, 1, 24, 16, 192, 192, 3, 1, 1, False), ('CK_SPLIT', 64, 192, 0, 3, 0)),
    ((2, 2, 1, 8, 8, 192, 192, 3, 2, 1, False), ('CK_SPLIT', 64, 192, 0, 3, 16)),
    ((2, 2, 1, 24, 16, 320, 192, 3, 1, 1, False), ('CK_SPLIT', 64, 192, 0, 5, 0)),
    ((2, 2, 1, 8, 8, 320, 192, 3, 2, 1, False), ('CK_SPLIT', 64, 192, 0, 5, 16)),
    ((2, 2, 1, 24, 16, 512, 192, 3, 1, 1, False), ('CK_SPLIT', 64, 192, 0, 9, 0)),
    ((2, 2, 1, 8, 8, 512, 192, 3, 2, 1, False), ('CK_SPLIT', 64, 192, 0, 9, 16)),
    ((2, 2, 3, 60, 52, 64, 16, 1, 1, 1, False), ('CK_SPLIT', 128, 64, 0, 1, 0)),
    ((2, 2, 32, 16, 16, 64, 16, 1, 1, 1, False), ('CK_SPLIT', 128, 64, 0, 1, 128)),
    ((2, 2, 22, 24, 16, 128, 16, 3, 1, 1, False), ('CK_SPLIT', 128, 64, 0, 2, 0)),
    ((2, 2, 32, 16, 16, 128, 16, 3, 1, 1, False), ('CK_SPLIT', 128, 64, 0, 2, 256)),
    ((2, 2, 22, 24, 16, 192, 16, 3, 1, 1, False), ('CK_SPLIT', 128, 64, 0, 3, 0)),
    ((2, 2, 32, 16, 16, 192, 16, 3, 1, 1, False), ('CK_SPLIT', 128, 64, 0, 3, 256)),
    ((2, 2, 31, 8, 8, 64, 512, 1, 1, 1, False), ('CK_SPLIT', 128, 128, 0, 1, 0)),
    ((2, 2, 16, 8, 16, 64, 512, 1, 1, 1, False), ('CK_SPLIT', 128, 128, 0, 1, 128)),
    ((2, 2, 1, 60, 52, 128, 1280, 3, 2, 1, False), ('CK_SPLIT', 128, 128, 0, 2, 0)),
    ((2, 2, 31, 8, 8, 128, 512, 3, 1, 1, False), ('CK_SPLIT', 128, 128, 0, 2, 64)),
    ((2, 2, 1, 60, 52, 192, 1280, 3, 2, 1, False), ('CK_SPLIT', 128, 128, 0, 3, 0)),
    ((2, 2, 31, 8, 8, 192, 512, 3, 1, 1, False), ('CK_SPLIT', 128, 128, 0, 3, 64)),
    ((2, 2, 21, 8, 8, 64, 960, 1, 1, 1, False), ('CK_SPLIT', 128, 160, 0, 1, 0)),
    ((2, 2, 32, 8, 16, 64, 320, 1, 1, 1, False), ('CK_SPLIT', 128, 160, 0, 1, 128)),
    ((2, 2, 11, 24, 16, 128, 320, 3, 1, 1, False), ('CK_SPLIT', 128, 160, 0, 2, 0)),
    ((2, 2, 21, 8, 8, 128, 960, 3, 1, 1, False), ('CK_SPLIT', 128, 160, 0, 2, 64)),
    ((2, 2, 11, 24, 16, 192, 320, 3, 1, 1, False), ('CK_SPLIT', 128, 160, 0, 3, 0)),
    ((2, 2, 21, 8, 8, 192, 960, 3, 1, 1, False), ('CK_SPLIT', 128, 160, 0, 3, 64)),
    ((2, 2, 3, 60, 52, 64, 192, 1, 1, 1, False), ('CK_SPLIT', 128, 192, 0, 1, 0)),
    ((2, 2, 32, 16, 16, 64, 192, 1, 1, 1, False), ('CK_SPLIT', 128, 192, 0, 1, 128)),
    ((2, 2, 22, 24, 16, 128, 192, 3, 1, 1, False), ('CK_SPLIT', 128, 192, 0, 2, 0)),
    ((2, 2, 32, 16, 16, 128, 192, 3, 1, 1, False), ('CK_SPLIT', 128, 192, 0, 2, 256)),
    ((2, 2, 22, 24, 16, 192, 192, 3, 1, 1, False), ('CK_SPLIT', 128, 192, 0, 3, 0)),
    ((2, 2, 32, 16, 16, 192, 192, 3, 1, 1, False), ('CK_SPLIT', 128, 192, 0, 3, 256)),
]
EDGE_REPRESENTATIVES = [
    ((0, 0, 16, 16, 32, 64, 768, 3, 1, 1, False), ('CK_HALO', 32, 128, 0, 1, 256)),
    ((0, 0, 1, 8, 8, 64, 64, 1, 1, 1, False), ('CK_IGEMM', 64, 64, 0, 1, 0)),
    ((0, 0, 1, 8, 8, 64, 16, 1, 1, 1, False), ('CK_IGEMM', 64, 64, 0, 1, 0)),
    ((0, 0, 1, 8, 8, 64, 64, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 1, 0)),
    ((0, 0, 1, 8, 8, 64, 16, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 1, 0)),
    ((0, 0, 1, 8, 8, 128, 64, 3, 1, 1, False), ('CK_IGEMM', 64, 64, 0, 2, 0)),
    ((0, 0, 1, 8, 8, 160, 64, 3, 1, 1, False), ('CK_IGEMM', 64, 64, 0, 2, 0)),
    ((0, 0, 1, 8, 8, 128, 16, 3, 1, 1, False), ('CK_IGEMM', 64, 64, 0, 2, 0)),
    ((0, 0, 1, 8, 8, 160, 16, 3, 1, 1, False), ('CK_IGEMM', 64, 64, 0, 2, 0)),
    ((0, 0, 1, 8, 8, 128, 64, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 2, 0)),
    ((0, 0, 1, 8, 8, 160, 64, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 2, 0)),
    ((0, 0, 1, 8, 8, 128, 16, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 2, 0)),
    ((0, 0, 1, 8, 8, 160, 16, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 2, 0)),
    ((0, 0, 1, 8, 8, 64, 128, 1, 1, 1, False), ('CK_IGEMM2', 64, 128, 0, 1, 0)),
    ((0, 0, 1, 8, 8, 64, 128, 3, 2, 1, False), ('CK_IGEMM2', 64, 128, 0, 1, 0)),
    ((0, 0, 1, 8, 8, 128, 128, 3, 1, 1, False), ('CK_IGEMM2', 64, 128, 0, 2, 0)),
    ((0, 0, 1, 8, 8, 160, 128, 3, 1, 1, False), ('CK_IGEMM2', 64, 128, 0, 2, 0)),
    ((0, 0, 1, 8, 8, 128, 128, 3, 2, 1, False), ('CK_IGEMM2', 64, 128, 0, 2, 0)),
    ((0, 0, 1, 8, 8, 160, 128, 3, 2, 1, False), ('CK_IGEMM2', 64, 128, 0, 2, 0)),
    ((0, 0, 28, 32, 64, 128, 512, 3, 2, 1, False), ('CK_IGEMM3', 256, 128, 0, 1, 0)),
    ((0, 0, 25, 24, 16, 128, 768, 3, 1, 1, False), ('CK_IGEMM3', 256, 128, 0, 1, 0)),
    ((0, 1, 1, 8, 8, 64, 64, 1, 1, 1, False), ('CK_IGEMM', 64, 64, 0, 1, 0)),
    ((0, 1, 1, 8, 8, 64, 16, 1, 1, 1, False), ('CK_IGEMM', 64, 64, 0, 1, 0)),
    ((0, 1, 1, 8, 8, 64, 64, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 1, 0)),
    ((0, 1, 1, 8, 8, 64, 16, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 1, 0)),
    ((0, 1, 1, 8, 8, 128, 64, 3, 1, 1, False), ('CK_IGEMM', 64, 64, 0, 2, 0)),
    ((0, 1, 1, 8, 8, 160, 64, 3, 1, 1, False), ('CK_IGEMM', 64, 64, 0, 2, 0)),
    ((0, 1, 1, 8, 8, 128, 16, 3, 1, 1, False), ('CK_IGEMM', 64, 64, 0, 2, 0)),
    ((0, 1, 1, 8, 8, 160, 16, 3, 1, 1, False), ('CK_IGEMM', 64, 64, 0, 2, 0)),
    ((0, 1, 1, 8, 8, 128, 64, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 2, 0)),
    ((0, 1, 1, 8, 8, 160, 64, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 2, 0)),
    ((0, 1, 1, 8, 8, 128, 16, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 2, 0)),
    ((0, 1, 1, 8, 8, 160, 16, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 2, 0)),
    ((0, 1, 1, 8, 8, 64, 128, 1, 1, 1, False), ('CK_IGEMM2', 64, 128, 0, 1, 0)),
    ((0, 1, 1, 8, 8, 64, 128, 3, 2, 1, False), ('CK_IGEMM2', 64, 128, 0, 1, 0)),
    ((0, 1, 1, 8, 8, 128, 128, 3, 1, 1, False), ('CK_IGEMM2', 64, 128, 0, 2, 0)),
    ((0, 1, 1, 8, 8, 160, 128, 3, 1, 1, False), ('CK_IGEMM2', 64, 128, 0, 2, 0)),
    ((0, 1, 1, 8, 8, 128, 128, 3, 2, 1, False), ('CK_IGEMM2', 64, 128, 0, 2, 0)),
    ((0, 1, 1, 8, 8, 160, 128, 3, 2, 1, False), ('CK_IGEMM2', 64, 128, 0, 2, 0)),
    ((0, 1, 28, 16, 32, 128, 512, 3, 1, 1, False), ('CK_IGEMM3', 256, 128, 0, 1, 0)),
    ((0, 1, 25, 24, 16, 128, 768, 3, 1, 1, False), ('CK_IGEMM3', 256, 128, 0, 1, 0)),
    ((1, 1, 1, 8, 8, 64, 64, 1, 1, 1, False), ('CK_IGEMM', 64, 64, 0, 1, 0)),
    ((1, 1, 1, 8, 8, 64, 16, 1, 1, 1, False), ('CK_IGEMM', 64, 64, 0, 1, 0)),
    ((1, 1, 1, 60, 52, 64, 64, 1, 1, 1, False), ('CK_IGEMM', 128, 64, 0, 1, 0)),
    ((1, 1, 1, 60, 52, 64, 16, 1, 1, 1, False), ('CK_IGEMM', 128, 64, 0, 1, 0)),
    ((1, 1, 1, 8, 8, 512, 64, 1, 1, 1, False), ('CK_IGEMM', 64, 64, 0, 2, 0)),
    ((1, 1, 1, 8, 8, 320, 64, 3, 1, 1, False), ('CK_IGEMM', 64, 64, 0, 11, 0)),
    ((1, 1, 1, 8, 8, 512, 16, 1, 1, 1, False), ('CK_IGEMM', 64, 64, 0, 2, 0)),
    ((1, 1, 1, 8, 8, 320, 16, 3, 1, 1, False), ('CK_IGEMM', 64, 64, 0, 11, 0)),
    ((1, 1, 1, 8, 8, 64, 64, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 2, 0)),
    ((1, 1, 1, 8, 8, 320, 64, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 11, 0)),
    ((1, 1, 1, 8, 8, 64, 16, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 2, 0)),
    ((1, 1, 1, 8, 8, 320, 16, 3, 2, 1, False), ('CK_IGEMM', 64, 64, 0, 11, 0)),
    ((1, 1, 1, 8, 8, 64, 128, 1, 1, 1, False), ('CK_IGEMM2', 64, 128, 0, 1, 0)),
    ((1, 1, 1, 60, 52, 64, 128, 1, 1, 1, False), ('CK_IGEMM2', 64, 128, 0, 1, 0)),
    ((1, 1, 1, 8, 8, 512, 128, 1, 1, 1, False), ('CK_IGEMM2', 64, 128, 0, 2, 0)),
    ((1, 1, 1, 8, 8, 320, 128, 3, 1, 1, False), ('CK_IGEMM2', 64, 128, 0, 11, 0)),
    ((1, 1, 1, 8, 8, 64, 128, 3, 2, 1, False), ('CK_IGEMM2', 64, 128, 0, 2, 0)),
    ((1, 1, 1, 8, 8, 320, 128, 3, 2, 1, False), ('CK_IGEMM2', 64, 128, 0, 11, 0)),
    ((2, 1, 1, 8, 8, 64, 64, 1, 1, 1, False), ('CK_SPLIT', 64, 64, 0, 1, 0)),
    ((2, 1, 1, 8, 8, 64, 16, 1, 1, 1, False), ('CK_SPLIT', 64, 64, 0, 1, 0)),
    ((2, 1, 1, 8, 8, 64, 64, 3, 2, 1, False), ('CK_SPLIT', 64, 64, 0, 1, 0)),
    ((2, 1, 1, 8, 8, 64, 16, 3, 2, 1, False), ('CK_SPLIT', 64, 64, 0, 1, 0)),
    ((2, 1, 1, 8, 8, 128, 64, 3, 1, 1, False), ('CK_SPLIT', 64, 64, 0, 2, 0)),
    ((2, 1, 1, 8, 8, 160, 64, 3, 1, 1, False), ('CK_SPLIT', 64, 64, 0, 2, 0)),
    ((2, 1, 1, 8, 8, 128, 16, 3, 1, 1, False), ('CK_SPLIT', 64, 64, 0, 2, 0)),
    ((2, 1, 1, 8, 8, 160, 16, 3, 1, 1, False), ('CK_SPLIT', 64, 64, 0, 2, 0)),
    ((2, 1, 1, 8, 8, 128, 64, 3, 2, 1, False), ('CK_SPLIT', 64, 64, 0, 2, 0)),
    ((2, 1, 1, 8, 8, 160, 64, 3, 2, 1, False), ('CK_SPLIT', 64, 64, 0, 2, 0)),
    ((2, 1, 1, 8, 8, 128, 16, 3, 2, 1, False), ('CK_SPLIT', 64, 64, 0, 2, 0)),
    ((2, 1, 1, 8, 8, 160, 16, 3, 2, 1, False), ('CK_SPLIT', 64, 64, 0, 2, 0)),
    ((2, 2, 16, 16, 32, 64, 768, 3, 1, 1, False), ('CK_HALO', 32, 128, 0, 1, 256)),
    ((2, 2, 4, 8, 8, 64, 128, 3, 1, 1, False), ('CK_HALO_SEG', 32, 128, 8, 3, 64)),
    ((2, 2, 4, 8, 8, 160, 128, 3, 1, 1, False), ('CK_HALO_SEG', 32, 128, 8, 7, 64)),
    ((2, 2, 4, 8, 8, 64, 192, 3, 1, 1, False), ('CK_HALO_SEG', 32, 128, 8, 3, 64)),
    ((2, 2, 4, 8, 8, 160, 192, 3, 1, 1, False), ('CK_HALO_SEG', 32, 128, 8, 7, 64)),
    ((2, 2, 1, 8, 8, 64, 64, 1, 1, 1, False), ('CK_SPLIT', 64, 64, 0, 1, 64)),
    ((2, 2, 1, 8, 8, 64, 16, 1, 1, 1, False), ('CK_SPLIT', 64, 64, 0, 1, 64)),
    ((2, 2, 1, 8, 8, 64, 64, 3, 2, 1, False), ('CK_SPLIT', 64, 64, 0, 1, 0)),
    ((2, 2, 1, 8, 8, 64, 16, 3, 2, 1, False), ('CK_SPLIT', 64, 64, 0, 1, 0)),
    ((2, 2, 1, 8, 8, 128, 64, 3, 1, 1, False), ('CK_SPLIT', 64, 64, 0, 2, 64)),
    ((2, 2, 1, 8, 8, 160, 64, 3, 1, 1, False), ('CK_SPLIT', 64, 64, 0, 2, 64)),
    ((2, 2, 1, 8, 8, 128, 16, 3, 1, 1, False), ('CK_SPLIT', 64, 64, 0, 2, 64)),
    ((2, 2, 1, 8, 8, 160, 16, 3, 1, 1, False), ('CK_SPLIT', 64, 64, 0, 2, 64)),
    ((2, 2, 1, 8, 8, 128, 64, 3, 2, 1, False), ('CK_SPLIT', 64, 64, 0, 2, 16)),
    ((2, 2, 1, 8, 8, 160, 64, 3, 2, 1, False), ('CK_SPLIT', 64, 64, 0, 2, 16)),
    ((2, 2, 1, 8, 8, 128, 16, 3, 2, 1, False), ('CK_SPLIT', 64, 64, 0, 2, 16)),
    ((2, 2, 1, 8, 8, 160, 16, 3, 2, 1, False), ('CK_SPLIT', 64, 64, 0, 2, 16)),
]
# TABLES-END


if __name__ == "__main__":
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if planner_env():
        raise SystemExit(f"unset {planner_env()} first: the tables are for the default knobs")
    print(regenerate())

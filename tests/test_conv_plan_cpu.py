"""The conv planner's class tables (tests/_conv_classes.py) against the planner itself, without a GPU: every row's expected plan is what
rs_conv_plan answers today, and the tables are closed over the grid - every class, and every edge combination, that any layer of the grid falls
into has a row, so tests/test_conv_plan_gpu.py runs the kernel of every plan the planner can make there.  No omission is allowed.

The planner reads its RS_IGEMM_* / RS_WINO* / RS_SPLIT* / RS_SPLITK_* knobs once per process: with one of them set the tables do not apply.

(The conv rows of Engine.profile_shapes() carry part, family, M, N and K - no plane, kernel size, stride or storage pair - so they cannot be
planned again and are not mapped onto the classes here.)

The closure fixture asks the planner about every layer of the grid, about 2.8 million calls through ctypes: it is most of this file's minute."""
import pytest

import _conv_classes as CC

pytestmark = pytest.mark.skipif(bool(CC.planner_env()), reason=f"planner knobs set in the environment: {CC.planner_env()}")

TABLES = {"class": (CC.REPRESENTATIVES, CC.class_key), "edge": (CC.EDGE_REPRESENTATIVES, CC.edge_key)}


@pytest.fixture(scope="module")
def grid_classes():
    best, edge = CC.classes_of_grid()
    return {"class": best, "edge": edge}


@pytest.mark.parametrize("which", sorted(TABLES))
def test_every_row_holds_todays_plan(which):
    table, keyfn = TABLES[which]
    rows = CC.rows(table)
    assert rows
    wrong = [(L, p, CC.plan_of(L)) for L, p in rows if CC.plan_of(L) != p]
    assert not wrong, wrong[:5]
    keys = [keyfn(L, p) for L, p in rows]
    assert len(set(keys)) == len(keys), "two rows of one class"
    from resshift_amd import ops

    for L, p in rows:
        assert p.kernel in ops.CONV_KERNELS[2:], p            # a kernel of the generic entry, not the Winograd one
        assert CC.gemm_dims(L)[0] <= CC.MAX_PIXELS, L


@pytest.mark.parametrize("which", sorted(TABLES))
def test_tables_are_closed_over_the_grid(grid_classes, which):
    """the classes of the whole grid == the classes of the table, and each row is the grid's cheapest layer of its class (ties: grid order)"""
    table, keyfn = TABLES[which]
    have = {keyfn(L, p): (L, p) for L, p in CC.rows(table)}
    want = grid_classes[which]
    missing, stale = sorted(set(want) - set(have)), sorted(set(have) - set(want))
    assert not missing and not stale, f"classes without a row: {missing}; rows of no class: {stale} - regenerate with python tests/_conv_classes.py"
    moved = [(k, have[k], want[k]) for k in want if have[k] != want[k]]
    assert not moved, moved[:5]


def test_the_fast_path_names_classes_as_the_class_key_does():
    """classes_of_grid forms its keys from the planner's raw integers; here 4000 layers drawn from the whole grid go the slow way - ops.conv_plan,
    class_key, edge_key - and every one must land in a class, and an edge combination, that has a row"""
    classes = {CC.class_key(L, p) for L, p in CC.rows(CC.REPRESENTATIVES)}
    edges = {CC.edge_key(L, p) for L, p in CC.rows(CC.EDGE_REPRESENTATIVES)}
    sample = CC.grid_sample(4000)
    assert len({(L.in_prec, L.out_prec, L.k, L.stride, L.up) for L in sample}) == len(CC.STORAGE) * len(CC.OPS)
    for L in sample:
        p = CC.plan_of(L)
        assert p is not None and CC.class_key(L, p) in classes and CC.edge_key(L, p) in edges, (L, p)


def test_residual_and_row_strides_keep_the_plan():
    """the tables' rows carry no residual (the planner asks of one only that ldres be a multiple of 8, so the residual-free layer wins every
    tie of the grid's order); the GPU sweep runs each edge row once more with a residual and as views into wider buffers - ld0 = C0 + 8,
    ldy = Cout + 8, ldres = Cout + 16, multiples of 8 - and that must be the same plan: for every row of both tables, each change alone and both"""
    for L, p in CC.rows(CC.REPRESENTATIVES) + CC.rows(CC.EDGE_REPRESENTATIVES):
        assert not L.res
        wide = (L.Cin + 8, L.Cout + 8, L.Cout + 16)
        for L2, ld in ((L, wide), (L._replace(res=True), None), (L._replace(res=True), wide)):
            assert CC.plan_of(L2, ld=ld) == p, (L2, ld, p)


def test_kernel_names_follow_the_enum():
    """ops.CONV_KERNELS is enum ConvKernel of csrc/common.h, name for name in its order: every kernel name the tables assert goes through it"""
    import os
    import re

    from resshift_amd import ops

    src = open(os.path.join(os.path.dirname(os.path.abspath(ops.__file__)), "csrc", "common.h")).read()
    body = re.search(r"enum\s+ConvKernel\s*\{([^}]*)\}", src).group(1)
    names = [e.strip() for e in body.split(",") if e.strip()]
    assert names[0].replace(" ", "") == "CK_NONE=0" and all("=" not in n for n in names[1:]), names   # counted up from 0, no gaps
    assert ("CK_NONE", *names[1:]) == ops.CONV_KERNELS


def test_plan_query_mirrors_the_entrys_routing():
    from resshift_amd import ops

    none = ops.ConvPlan("CK_NONE", 0, 0, 0, 0, 0)
    assert ops.conv_plan(2, 16, 16, 6, 160, 3, ops.F16) == none        # the direct kernels' layers: Cin % 8, Cout <= 8
    assert ops.conv_plan(1, 16, 16, 512, 8, 3, ops.F16) == none
    assert ops.conv_plan(1, 16, 16, 64, 64, 3, ops.F32, ops.F16) is None   # a storage pair no kernel takes
    assert ops.conv_plan(3, 8, 8, 64, 48, 3, ops.F16).kernel == "CK_IGEMM"

"""GPU parity on crafted weights: the reduced-cell components (k_cc_local, k_cc_step), fixReducedRegionBoundaries as a fixed point per sweep
(k_fix_eval, k_fix_apply), fixSmallReducedRegions and the per-tile kernels that walk a region's bounding box, on the case table of
classification_cases.py — chains of fixes by cells demoted earlier in the same sweep, several applying sweeps, regions emptied and removed,
two regions in one tile with overlapping boxes, regions that do not fill their box, tile-local components longer than the local kernel's pass
limit.  The library and the CPU oracle are given the same weights; the integer state is compared bit for bit, what the regions feed with the
tolerances of test_gpu_parity.py (helpers.check_*).  test_classification_cases_cpu.py asserts that the cases reach all this.  Single domain only.
"""
import numpy as np
import pytest

from polystokes_amd import _abi as abi
from polystokes_amd import scenes

import children
import classification_cases as cc
from helpers import check_rhs_and_operator, check_solve, check_stencil_blocks, check_tile_blocks

pytestmark = pytest.mark.gpu

INTEGER_KINDS = ("LiquidWeights", "FluidWeights", "Labels", "ActiveIndices", "ReducedIndices")
LABEL_KINDS = ("Labels", "ActiveIndices", "ReducedIndices")


def setup_only(p):
    """the same parameters without a solve: setup, the valid fields, the velocity left alone (HDK_PolyStokes.C:513, 566-583)"""
    q = type(p).from_buffer_copy(p)
    q.doSolve, q.keepNonConvergedResults = 0, 0
    return q


def integer_state(s, valid=None):
    """dimData, the 7 x 5 weight / label / index arrays and (after a step) the three valid fields of a Solver or an Oracle"""
    st = {"dimData": np.array(list(s.stats.dimData))}
    for g in abi.SAMPLE_NAMES:
        for kind in INTEGER_KINDS:
            st[g + kind] = s.array(g + kind)
    for a in range(3):
        st["valid" + "XYZ"[a]] = np.asarray(valid[a], np.float32).ravel() if valid is not None else s.array("valid" + "XYZ"[a])
    return st


def assert_same_state(a, b, what, keys=None):
    for k in (keys if keys is not None else b):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differs in {(a[k] != b[k]).sum()} entries"


def run_setup(solver, name):
    """step a case without its solve on a Solver: its integer state"""
    sc, p = cc.build(name)
    rc = solver.step(sc, setup_only(p))
    assert rc == abi.INCOMPLETE, (name, rc)
    return integer_state(solver, solver.valid)


@pytest.fixture(scope="module")
def gpu():
    import polystokes_amd
    s = polystokes_amd.Solver(0)
    yield s
    s.close()


# ---- the integer state of every case --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.CASES))
def test_integer_state_is_bit_exact(gpu, oracle_mod, name):
    sc, p = cc.build(name)
    q = setup_only(p)
    o = oracle_mod.Oracle()
    ro = o.run(sc, q)
    rc = gpu.step(sc, q)
    assert rc == ro == abi.INCOMPLETE, name
    assert list(gpu.stats.dimData) == list(o.stats.dimData), name
    assert_same_state(integer_state(gpu, gpu.valid), integer_state(o), name)
    for a in range(3):                                             # no solve: the velocity is the input's
        assert np.array_equal(gpu.vel[a], sc.vel[a]), name


# ---- what the regions feed: tile blocks, stencil blocks, the operator, the solve --------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_fed():
    import polystokes_amd
    s = polystokes_amd.Solver(0)
    yield s
    s.close()


@pytest.fixture(scope="module", params=cc.FEED_CASES)
def fed(request, gpu_fed, oracle_mod):
    sc, p = cc.build(request.param)
    o = oracle_mod.Oracle()
    o.run(sc, p, solve=True)
    gpu_fed.upload(sc, p)
    gpu_fed.setup()
    return request.param, sc, p, o, gpu_fed


def test_fed_regions_are_the_oracles(fed):
    name, sc, p, o, g = fed
    assert o.nRegions >= 2 and g.nRegions == o.nRegions, name
    assert list(g.stats.dimData) == list(o.stats.dimData), name
    for s in abi.SAMPLE_NAMES:
        for kind in LABEL_KINDS:
            assert np.array_equal(g.array(s + kind), o.array(s + kind)), (name, s + kind)


def test_fed_tile_blocks_match(fed):
    check_tile_blocks(*fed)


def test_fed_stencil_blocks_match(fed):
    check_stencil_blocks(*fed)


def test_fed_rhs_and_operator_match(fed):
    check_rhs_and_operator(*fed)


def test_fed_solve_matches(fed):
    name, sc, p, o, g = fed
    assert o.result == abi.SUCCESS and o.stats.solveData[1] > 10, name          # (a solve that iterates: the velocity varies in space)
    check_solve(*fed)


# ---- switches read once per process: a child runs the cases and stores their state ------------------------------------------------------------
_CHILD = r'''
out, names = sys.argv[1], sys.argv[2:]
import classification_cases as cc
import test_gpu_classification as t
s = polystokes_amd.Solver(0)
data = {}
for name in names:
    if name.startswith("blocks:"):          # set up with the solve's own parameters: the tile blocks
        name = name[7:]
        sc, p = cc.build(name)
        s.upload(sc, p)
        s.setup()
        for k in ("reducedMassMatrices", "reducedViscosityMatrices", "Inv_Mr_plus_2JDtuDJ"):
            data[name + "/" + k] = s.array(k)
        data[name + "/R"] = np.int64(s.nRegions)
    else:
        for k, v in t.run_setup(s, name).items():
            data[name + "/" + k] = v
np.savez(out, **data)
s.close()
'''


def run_child(tmp_path, env, names):
    out = str(tmp_path / "child.npz")
    # (the lab build names a test-only switch that changes results when it finds it set)
    children.run_python(_CHILD, out, *names, limit=300, env=env, expect=[f"{k}={v} is active" for k, v in env.items() if k == "PS_DEBUG_POISON"])
    return np.load(out)


def state_keys():
    return ["dimData"] + [g + k for g in abi.SAMPLE_NAMES for k in LABEL_KINDS] + ["valid" + a for a in "XYZ"]


def test_grid_wide_component_passes_alone_give_the_same_labels(gpu, tmp_path):
    """PS_CC_LOCAL=0: k_cc_step alone, without the tile-local pass in LDS, on cases in which the local pass runs by default (tiles on,
    padding >= 1, 4 <= B <= 23): all label and index arrays bit-identical."""
    names = ["walls_18x17x19_t6p1", "maze_t8p1", "serpentine_16p1", "serpentine_16p1_mirrored_linear", "interlocked_t12p1"]
    alt = run_child(tmp_path, {"PS_CC_LOCAL": "0"}, names)
    for name in names:
        sc, p = cc.build(name)
        assert p.doTile and p.tilePadding >= 1 and 4 <= p.tileSize <= 23
        mine = run_setup(gpu, name)
        assert_same_state({k: alt[name + "/" + k] for k in state_keys()}, mine, name + " without the local pass", state_keys())


def test_poisoned_scratch_changes_nothing(gpu, tmp_path):
    """PS_DEBUG_POISON=1 fills whatever the context's allocator hands out.  The boundary fix reuses cellScratch[0..2] across the component pass
    and its sweeps (labels, root ranks and link bits, then the two fix-flag buffers): the 15-sweep walls case and the serpentines, in which
    both the local and the grid-wide component passes do work, give the same bits."""
    names = ["walls_12x10x14_linear", "serpentine_16p1", "serpentine_23p1"]
    alt = run_child(tmp_path, {"PS_DEBUG_POISON": "1"}, names)
    for name in names:
        mine = run_setup(gpu, name)
        assert_same_state({k: alt[name + "/" + k] for k in state_keys()}, mine, name + " poisoned", state_keys())


def test_two_regions_in_a_tile_without_shared_tile_blocks(gpu, tmp_path):
    """PS_NO_TILE_CLASSES=1 on an interlocked tiled case (two regions per tile, overlapping boxes): every tile sums its own blocks.  Mr is never
    shared: bit-identical; K and BInv <= 1e-12 relative per block, as in test_shared_tile_blocks_equal_the_tiles_own_sums."""
    name = "interlocked_t12p2"
    alt = run_child(tmp_path, {"PS_NO_TILE_CLASSES": "1"}, ["blocks:" + name])
    sc, p = cc.build(name)
    gpu.upload(sc, p)
    gpu.setup()
    R = gpu.nRegions
    assert R == int(alt[name + "/R"]) and R >= 8
    assert np.array_equal(gpu.array("reducedMassMatrices"), alt[name + "/reducedMassMatrices"])
    for nm in ("reducedViscosityMatrices", "Inv_Mr_plus_2JDtuDJ"):
        A, B = gpu.array(nm).reshape(R, -1), alt[name + "/" + nm].reshape(R, -1)
        rel = np.abs(A - B).max(axis=1) / np.abs(B).max(axis=1)
        assert rel.max() <= 1e-12, (nm, rel.max())


# ---- one context through regionCount 0 and back ----------------------------------------------------------------------------------------------
def test_one_context_through_no_regions_and_back():
    """maze -> cavity(16) -> walls -> maze on ONE context: the region count goes 18 -> 1 -> 0 -> 18, and bbox, keep and remap are reallocated
    at other sizes.  Every setup equals the one of a fresh context."""
    import polystokes_amd

    def step(s, what):
        if what == "cavity16":
            sc, p = scenes.cavity(16)
            rc = s.step(sc, setup_only(p))
            assert rc == abi.INCOMPLETE
            return integer_state(s, s.valid)
        return run_setup(s, what)

    seq = ["maze_t8p1", "cavity16", "walls_12x10x14_linear", "maze_t8p1"]
    fresh = {}
    for what in set(seq):
        s = polystokes_amd.Solver(0)
        try:
            fresh[what] = step(s, what)
        finally:
            s.close()
    regions = [int(fresh[w]["dimData"][24]) for w in seq]
    assert regions[0] >= 5 and regions[1] >= 1 and regions[2] == 0 and regions[3] == regions[0], regions
    s = polystokes_amd.Solver(0)
    try:
        for n, what in enumerate(seq):
            assert_same_state(step(s, what), fresh[what], f"step {n} ({what}) on a used context")
    finally:
        s.close()

"""Collider placement and painting (ps_place_colliders, ps_paint_collider_velocities) on slab and brick ranks, on the GPU.  A rank runs both
rules on its own grid from the orig of its own upload (partition.local_orig): every rank of an in-process Group is compared byte for byte
with the two numpy restatements run on the rank's cut arrays (collider_decomposition_cases.rank_expected), the two views of every cut with
each other, and a step after the ranks' own placement with a step of ranks that were uploaded the global restatement's fields.
test_collider_decomposition_cpu.py shows on the restatements alone what these tests rely on: where a rank's result equals the global
one, the one plane per halo side where the paint's rule makes it differ, and that the cases tell the partition helper from its near misses."""
import os
import sys

import numpy as np
import pytest

import polystokes_amd
from polystokes_amd import _abi as abi
from polystokes_amd import partition

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import children  # noqa: E402
import collider_decomposition_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

BOX = sorted(cases.CASES)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_rank(s, want, c, what):
    col, idf, placed, grids, faces = cases.rank_arrays(s)
    wcol, widf, wplaced, wgrids, wfaces = want
    print(what, "cells", placed.tolist(), "faces", faces.tolist())
    assert np.array_equal(placed, wplaced), (what, placed.tolist(), wplaced.tolist())
    bad = np.argwhere(bits(col) != bits(wcol))
    assert bad.size == 0, (what, "collision", len(bad), bad[:4].tolist())
    bad = np.argwhere(idf != widf)
    assert bad.size == 0, (what, "ids", len(bad), bad[:4].tolist())
    for a in range(3):
        bad = np.argwhere(bits(grids[a]) != bits(wgrids[a]))
        assert bad.size == 0, (what, "collisionvel", a, len(bad), bad[:4].tolist())
    assert np.array_equal(faces, wfaces), (what, faces.tolist(), wfaces.tolist())
    assert s.array("colliderPoseTable").tobytes() == c.poses.tobytes()                   # the global tables, the same on every rank
    assert s.array("colliderMotionTable").tobytes() == c.motions.tobytes()
    assert int(s.array("colliderPlacement")[0]) == len(c.shapes) and int(s.array("colliderMotions")[0]) == len(c.motions)


# ---- 1. every rank against the restatement on its own grid ---------------------------------------------------------------------------------
@pytest.mark.parametrize("when", ["before_cut", "after_cut"])
@pytest.mark.parametrize("case", BOX)
def test_rank_grids_equal_the_restatement(case, when):
    """host forms: the rank's cut of the ids, the global pose and motion tables"""
    c = cases.build(case)
    grp = cases.run_group(case, when)
    try:
        for r, (s, want) in enumerate(zip(grp.ranks, cases.expected(case))):
            assert_rank(s, want, c, "%s %s rank %d" % (case, when, r))
            assert s.memory_stats()["deferred_bytes"] == 0
    finally:
        grp.close()


def test_device_forms_leave_what_the_host_forms_leave():
    """box_xz in a child process that imports torch first and hands ps_place_colliders_device / ps_paint_collider_velocities_device the
    tables as torch tensors on torch's current stream, on every rank: one digest over every rank's grids and counters, identical to the
    host forms' of an in-process group here and to the restatement's"""
    case = "box_xz"
    pr = children.run_script("collider_decomposition_cases.py", "ranks_torch", case, limit=300, drop=("PS_LIB",))
    grp = cases.run_group(case)
    try:
        host = cases.group_digest(grp)
    finally:
        grp.close()
    assert dict(pr.digests()) == {case: host}, pr.output[-2000:]
    assert host == cases.expected_digest(case)


# ---- 2. the two views of a cut ---------------------------------------------------------------------------------------------------------------
def overlap(ga, gb, face_axis=None):
    """the index tuples of ranks a and b for the cells (or the faces of face_axis) that both hold, or None"""
    ia, ib = [], []
    for q in (2, 1, 0):
        e = int(face_axis == q)
        lo, hi = max(ga.origin[q], gb.origin[q]), min(ga.origin[q] + ga.n[q], gb.origin[q] + gb.n[q]) + e
        if hi - e <= lo:                                           # (no cell of this axis is held by both)
            return None
        ia.append(slice(lo - ga.origin[q], hi - ga.origin[q]))
        ib.append(slice(lo - gb.origin[q], hi - gb.origin[q]))
    return tuple(ia), tuple(ib)


@pytest.mark.parametrize("case", BOX)
def test_both_views_of_a_cut_agree(case):
    """Every pair of ranks, every cell and face both hold: the placed collision, the ids and the painted velocity are equal, the ranks'
    arrays against each other.  Excepted: a face on the outermost plane of a halo side of either rank (Geometry.outer_planes), which has
    one cell there and two on the other rank."""
    c = cases.build(case)
    grp = cases.run_group(case)
    try:
        got = [cases.rank_arrays(s) for s in grp.ranks]
    finally:
        grp.close()
    shared_cells = shared_faces = excepted = 0
    for a in range(c.world):
        for b in range(a + 1, c.world):
            ga, gb = c.geo[a], c.geo[b]
            ov = overlap(ga, gb)
            if ov is None:
                continue
            ia, ib = ov
            assert np.array_equal(bits(got[a][0][ia]), bits(got[b][0][ib])), (case, a, b, "collision")
            assert np.array_equal(got[a][1][ia], got[b][1][ib]), (case, a, b, "ids")
            shared_cells += got[a][0][ia].size
            for ax in range(3):
                fa, fb = overlap(ga, gb, ax)
                skip = ga.outer_planes(ax)[fa] | gb.outer_planes(ax)[fb]
                va, vb = bits(got[a][3][ax][fa]), bits(got[b][3][ax][fb])
                bad = np.argwhere((va != vb) & ~skip)
                assert bad.size == 0, (case, a, b, ax, len(bad), bad[:4].tolist())
                shared_faces += int((~skip).sum())
                excepted += int(((va != vb) & skip).sum())
    print(case, "cells held twice", shared_cells, "faces held twice", shared_faces, "differing on the excepted planes", excepted)
    assert shared_cells > 0 and shared_faces > 0 and excepted > 0


# ---- 3. the block cull on a local grid -------------------------------------------------------------------------------------------------------
def test_without_the_cull_every_rank_leaves_the_same():
    """PS_DEBUG_SHAPE_CULL=0 (lab build) lets every collider into every block of every rank: a collider that reaches only a halo block of a
    rank (volume 2 of the case) is placed there either way"""
    case = "box_xz"
    pr = children.run_script("collider_decomposition_cases.py", "ranks", case, limit=300, env={"PS_DEBUG_SHAPE_CULL": "0"}, drop=("PS_LIB",),
                             expect=["PS_DEBUG_SHAPE_CULL=0 is active"])
    assert dict(pr.digests()) == {case: cases.expected_digest(case)}, pr.output[-2000:]


# ---- 4. a step after the ranks' own placement ---------------------------------------------------------------------------------------------------
def group_step(dims, world, sc, p, shapes=None, hook=None):
    """One step of a fresh group; returns what the comparisons read."""
    grp = polystokes_amd.Group(world, dims=dims)
    try:
        if shapes is not None:
            for s in grp.ranks:
                assert s.set_collider_shapes(shapes) == abi.SUCCESS, s.last_error()
        rc = grp.solve_scene(sc, p, per_rank=hook)
        return {"rc": int(rc), "iters": int(grp.stats.solveData[1]), "vel": [v.copy() for v in grp.vel], "valid": [v.copy() for v in grp.valid],
                "x": [s.array("solutionVector").tobytes() for s in grp.ranks], "labels": [s.array("centerLabels").copy() for s in grp.ranks],
                "halo_labels": [s.dist_stats()["halo_label_changes"] for s in grp.ranks], "parts": grp.slabs}
    finally:
        grp.close()


def same_bytes(u, v):
    return (u["rc"] == v["rc"] and u["iters"] == v["iters"] and u["x"] == v["x"]
            and all(np.array_equal(a, b) for a, b in zip(u["labels"], v["labels"]))
            and all(a.tobytes() == b.tobytes() for a, b in zip(u["vel"] + u["valid"], v["vel"] + v["valid"])))


def within_the_single_domain_bound(got, want_rc, want_iters, want_vel, want_valid, tol, what):
    assert got["rc"] == want_rc == abi.SUCCESS, (what, got["rc"], want_rc)
    assert abs(want_iters - got["iters"]) <= max(2, 0.02 * want_iters), (what, want_iters, got["iters"])
    for a in range(3):
        assert np.array_equal(got["valid"][a], want_valid[a]), (what, a)
        scale = max(np.abs(want_vel[a]).max(), 1e-30)
        assert np.abs(got["vel"][a] - want_vel[a]).max() <= 20 * tol * scale, (what, a)


@pytest.mark.parametrize("case", sorted(cases.STEP_CASES))
def test_step_after_the_ranks_placement(case):
    """Run (a): the single domain uploads, places, paints and steps.  Run (b): every rank of the group does the same on its part.  Run (c):
    ranks that are uploaded the global restatement's collision and collisionvel, cut by the partition, and neither place nor paint.
    (b) against (a): the assertions of the group tests against the single domain.  (b) against (c): byte for byte — the iteration count,
    every rank's solutionVector and labels, the merged velocity and valid flags, the halo labels the owners replaced; the inputs of the
    two differ on the outermost face plane of every halo side alone, so the solve does not read that plane.  (c) is run twice first: were
    an in-process group not reproducible run to run, (b) is held against (c) to the single-domain bound instead."""
    dims, world = cases.STEP_CASES[case]
    sc, p, shapes, poses, motions = cases.step_scene()
    hook = cases.step_hook(shapes, poses, motions)
    single = polystokes_amd.Solver(0)
    try:
        assert single.set_collider_shapes(shapes) == abi.SUCCESS
        single.upload(sc, p)
        hook(single, None, sc)
        rc_a = int(single.step_device())
        single.download()
        iters_a, vel_a, valid_a = int(single.stats.solveData[1]), single.vel, single.valid
        labels_a = single.array("centerLabels").reshape(sc.nz, sc.ny, sc.nx)
    finally:
        single.close()
    b = group_step(dims, world, sc, p, shapes, hook)
    print(case, "single", rc_a, iters_a, "ranks place", b["rc"], b["iters"])
    within_the_single_domain_bound(b, rc_a, iters_a, vel_a, valid_a, p.tolerance, "(b) against (a)")
    for r, part in enumerate(b["parts"]):                          # every owned label equals the global classification
        g = cases.Geometry(part, (sc.nx, sc.ny, sc.nz))
        own = g.owned_cells()
        assert np.array_equal(b["labels"][r].reshape(own.shape)[own], g.cut(labels_a)[own]), (case, r)
    sc_c, p_c, placed, faces = cases.placed_step_scene()
    c1 = group_step(dims, world, sc_c, p_c)
    c2 = group_step(dims, world, sc_c, p_c)
    reproducible = same_bytes(c1, c2)
    print(case, "pre-placed", c1["rc"], c1["iters"], "twice the same bytes:", reproducible, "(b) == (c):", same_bytes(b, c1),
          "halo labels replaced", b["halo_labels"], c1["halo_labels"])
    if reproducible:
        assert b["rc"] == c1["rc"] and b["iters"] == c1["iters"], (b["iters"], c1["iters"])
        assert b["halo_labels"] == c1["halo_labels"]
        for r in range(world):
            assert np.array_equal(b["labels"][r], c1["labels"][r]), (case, r, "centerLabels")
            assert b["x"][r] == c1["x"][r], (case, r, "solutionVector")
        for a in range(3):
            assert b["vel"][a].tobytes() == c1["vel"][a].tobytes() and b["valid"][a].tobytes() == c1["valid"][a].tobytes(), (case, a)
    else:
        within_the_single_domain_bound(b, c1["rc"], c1["iters"], c1["vel"], c1["valid"], p.tolerance, "(b) against (c)")
    assert reproducible, "two identical runs of an in-process group differ: (b) was held against (c) to the single-domain bound only"


# ---- 5. lifetime on a rank ---------------------------------------------------------------------------------------------------------------------
def test_lifetime_of_the_arrays_on_a_rank():
    case = "box_no_ids"                                            # no id field: the placement creates it on each rank
    c = cases.build(case)
    names = ("colliderPlacement", "colliderMotions", "collisionField", "colliderCellIds", "colliderPlacedCells", "colliderMotionFaces") + cases.GRID_ARRAYS
    grp = cases.run_group(case, "before_cut")
    try:
        for r, (s, part, want) in enumerate(zip(grp.ranks, grp.slabs, cases.expected(case))):
            before = {n: s.array(n).tobytes() for n in names}
            s.set_brick(part)                                      # again, after place and paint: the arrays stay, byte for byte
            assert {n: s.array(n).tobytes() for n in names} == before, r
            assert_rank(s, want, c, "%s after set_brick rank %d" % (case, r))
            with pytest.raises(polystokes_amd.PolyStokesError, match="air pockets need a single domain"):
                s.label_air_pockets()
            assert s.memory_stats()["deferred_bytes"] == 0         # ps_memory_stats entry 2
        one = grp.ranks[1]                                         # a second upload on one rank erases its arrays, and only its
        one.upload(cases.local(case, grp.slabs[1])[0], c.params)
        for n in ("colliderPlacement", "colliderMotions", "colliderCellIds", "collisionField"):
            with pytest.raises(KeyError):
                one.array(n)
        assert int(one.array("colliderShapes")[0]) == len(c.shapes)
        assert int(grp.ranks[0].array("colliderPlacement")[0]) == len(c.shapes) and int(grp.ranks[2].array("colliderMotions")[0]) == len(c.motions)
        assert all(s.memory_stats()["deferred_bytes"] == 0 for s in grp.ranks)
        # ... and the rank places and paints again on the fresh upload, to the same bytes
        cases.place_and_paint(case)(one, grp.slabs[1], None)
        one.set_brick(grp.slabs[1])
        assert_rank(one, cases.expected(case)[1], c, "%s rank 1 after a second upload" % case)
    finally:
        grp.close()

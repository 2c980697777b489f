"""Collider shapes (ps_set_collider_shapes, ps_place_colliders) on the GPU.  The placed collision field, the id field and the counters are a
function of the upload — collision SDF, ids, orig, dx, negateCollision — the volumes and the poses, restated in numpy
(collider_shapes_ref.py): the device is compared with the restatement byte for byte, and a step after a placement with a step of a fresh
context uploaded with the restatement's field.  test_collider_shapes_ref_cpu.py shows that the shared cases tell the rule from its near
misses."""
import ctypes
import os
import sys

import numpy as np
import pytest

import polystokes_amd
from polystokes_amd import _abi as abi
from polystokes_amd import _hip
from polystokes_amd import scenes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import children  # noqa: E402
import collider_motions_ref as motions_ref  # noqa: E402
import collider_shapes_cases as cases  # noqa: E402
import collider_shapes_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


def assert_placed(s, col, idf, counters, what=""):
    c, i, n = cases.placed(s)
    print(what, "cells device", n.tolist(), "reference", np.asarray(counters).tolist())
    assert np.array_equal(n, counters), what
    bad = np.argwhere(c.view(np.uint32) != col.view(np.uint32))
    assert bad.size == 0, (what, "collision", len(bad), bad[:4].tolist())
    bad = np.argwhere(i != idf)
    assert bad.size == 0, (what, "ids", len(bad), bad[:4].tolist())


def on_device(tab):
    return _hip.DeviceBuffer.from_numpy(np.ascontiguousarray(tab, np.float64).view(np.float32))


def snapshot(s):
    return [s.array(n).tobytes() for n in cases.ARRAYS]


# ---- 1. against the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(cases.CASES))
def test_placement_equals_the_restatement(case):
    sc, p, ids, shapes, poses, col, idf, counters = cases.build(case)
    s = polystokes_amd.Solver(0)
    try:
        cases.upload_and_place(s, case)                                            # host ids, host poses
        assert int(s.array("colliderShapes")[0]) == len(shapes) == int(s.array("colliderPlacement")[0])
        assert s.array("colliderPoseTable").tobytes() == poses.tobytes()
        assert_placed(s, col, idf, counters, "host")
        # ids from device memory in z-fastest layout, the poses from device memory
        s.upload(sc, p)
        dev_ids = None
        if ids is not None:
            dev_ids = _hip.DeviceBuffer.from_numpy(np.ascontiguousarray(ids.transpose(2, 1, 0)).view(np.float32))
            assert s.upload_collider_ids_device(dev_ids, abi.LAYOUT_Z_FASTEST) == abi.SUCCESS, s.last_error()
        dev = on_device(poses)
        assert s.place_colliders_device(dev, len(shapes)) == abi.SUCCESS, s.last_error()
        assert_placed(s, col, idf, counters, "device")
        dev.close()
        if dev_ids is not None:
            dev_ids.close()
    finally:
        s.close()


def _child(env_extra, names):
    pr = children.run_script("collider_shapes_cases.py", "place", *names, limit=600, env=env_extra, drop=("PS_LIB",),
                             expect=["%s=%s is active" % kv for kv in env_extra.items()])  # the child read the switch
    want = {c: cases.digest(cases.build(c)[5:8]) for c in names}
    assert dict(pr.digests()) == want, pr.output[-2000:]


def test_without_the_cull_the_outputs_are_identical():
    """PS_DEBUG_SHAPE_CULL=0 (lab build) lets every collider into every block: the per-cell test alone decides, and nothing changes"""
    _child({"PS_DEBUG_SHAPE_CULL": "0"}, sorted(cases.CASES))


def test_poisoned_buffers_change_nothing():
    """PS_DEBUG_POISON=1 fills whatever a buffer allocation hands out with 0xff: a kernel that read a word nobody wrote would show"""
    _child({"PS_DEBUG_POISON": "1"}, ["three_orig", "count64", "spacings"])


# ---- 2. a step after a placement -----------------------------------------------------------------------------------------------------------
def test_step_after_placement_equals_a_step_of_the_placed_upload():
    sc, p, shapes, poses, motions = cases.step_scene()
    col, idf, counters = ref.place(sc.collision, None, shapes, poses, (0.0, 0.0, 0.0), sc.dx, 1)
    assert (counters[:2] > 50).all()
    cvel, faces = motions_ref.paint(col, idf, motions, (0.0, 0.0, 0.0), sc.dx, 1, sc.collisionvel)
    s = polystokes_amd.Solver(0)
    try:
        assert s.set_collider_shapes(shapes) == abi.SUCCESS
        s.upload(sc, p)
        assert s.place_colliders(poses) == abi.SUCCESS, s.last_error()
        assert_placed(s, col, idf, counters, "before the step")
        assert s.paint_collider_velocities(motions) == abi.SUCCESS, s.last_error()
        assert np.array_equal(s.array("colliderMotionFaces"), faces)               # the paint read the placed field and the created ids
        got = cases.step_outcome(s)
        assert_placed(s, col, idf, counters, "after the step")                     # the step kept the arrays and the buffers
    finally:
        s.close()
    sc2, p2 = scenes.spheres(32, tile=8)
    p2.preconditioner = abi.PRE_DIAGONAL
    sc2.collision = col.copy()
    s = polystokes_amd.Solver(0)
    try:
        s.upload(sc2, p2)
        assert s.upload_collider_ids(idf) == abi.SUCCESS
        assert s.paint_collider_velocities(motions) == abi.SUCCESS
        want = cases.step_outcome(s)
    finally:
        s.close()
    print("step", got[:3])
    assert got[0] == abi.SUCCESS and got[1] == abi.SUCCESS and got[:3] == want[:3], (got[:3], want[:3])
    assert got[3] == want[3] and got[4] == want[4]


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refused_shapes_keep_the_old_ones():
    sc, p, ids, shapes, poses, col, idf, counters = cases.build("three_negate")
    s = polystokes_amd.Solver(0)
    try:
        assert s.set_collider_shapes(shapes) == abi.SUCCESS                        # before any upload
        assert int(s.array("colliderShapes")[0]) == 3
        sdf, h, o = shapes[1]

        def refused(bad, why):
            assert s.set_collider_shapes(bad) == abi.INVALID, why
            assert why in s.last_error(), (why, s.last_error())
            assert "PS_" not in s.last_error()
            assert int(s.array("colliderShapes")[0]) == 3
        refused([shapes[0]] * 65, "count outside 0..64")
        refused([shapes[0], (np.zeros((3, 1, 4), np.float32), h, o), (sdf, -1.0, o)], "shape 1: extent outside 2..1022")
        refused([shapes[0], (np.zeros((2, 2, 1023), np.float32), h, o)], "shape 1: extent outside 2..1022")
        for bad_h in (0.0, -0.5, np.inf, np.nan):
            refused([shapes[0], shapes[1], (sdf, bad_h, o)], "shape 2: spacing not positive and finite")
        refused([(sdf, h, (0.0, np.nan, 0.0)), shapes[1]], "shape 0: origin not finite")
        tab = (abi.ColliderShape * 2)()
        for k in range(2):
            tab[k].n[0], tab[k].n[1], tab[k].n[2], tab[k].h = 2, 2, 2, 0.1
        tab[0].sdf = np.zeros(8, np.float32).ctypes.data
        assert s.L.ps_set_collider_shapes(s.h, ctypes.byref(abi.ColliderShapes(2, tab))) == abi.INVALID
        assert "shape 1: no samples" in s.last_error() and int(s.array("colliderShapes")[0]) == 3
        v = sdf.copy()
        v.ravel()[17] = np.nan
        v.ravel()[40] = np.inf
        w = shapes[2][0].copy()
        w.ravel()[0] = np.nan
        refused([shapes[0], (v, h, o), (w, 0.11, o)], "shape 1: non-finite value at sample 17")
        # the old shapes still place
        s.upload(sc, p)
        assert s.upload_collider_ids(ids) == abi.SUCCESS
        assert s.place_colliders(poses) == abi.SUCCESS, s.last_error()
        assert_placed(s, col, idf, counters, "after the refusals")
        # dropping them: no array, and a placement is refused
        for drop in (None, []):
            assert s.set_collider_shapes(drop) == abi.SUCCESS
            with pytest.raises(KeyError):
                s.array("colliderShapes")
        assert s.L.ps_set_collider_shapes(s.h, ctypes.byref(abi.ColliderShapes(0, None))) == abi.SUCCESS
        assert s.place_colliders(poses) == abi.INVALID and "no shapes set" in s.last_error()
    finally:
        s.close()


def test_refused_placements_write_nothing():
    case = "three_negate"
    sc, p, ids, shapes, poses, col, idf, counters = cases.build(case)
    s = polystokes_amd.Solver(0)
    try:
        dev = on_device(poses)
        assert s.place_colliders(poses) == abi.INVALID and "call ps_upload_fields first" in s.last_error()
        assert s.place_colliders_device(dev, 3) == abi.INVALID and "call ps_upload_fields first" in s.last_error()
        s.upload(sc, p)
        assert s.place_colliders(poses) == abi.INVALID and "no shapes set" in s.last_error()
        assert s.place_colliders_device(dev, 3) == abi.INVALID and "no shapes set" in s.last_error()
        cases.upload_and_place(s, case)
        before = snapshot(s)

        def unchanged(why):
            assert why in s.last_error(), (why, s.last_error())
            assert snapshot(s) == before, why
        assert s.L.ps_place_colliders(s.h, None) == abi.INVALID
        unchanged("poses is null")
        assert s.L.ps_place_colliders(s.h, ctypes.byref(abi.ColliderPoses(3, None))) == abi.INVALID
        unchanged("pose is null")
        assert s.place_colliders_device(None, 3) == abi.INVALID
        unchanged("pose is null")
        for count in (2, 4, 0):
            assert s.L.ps_place_colliders(s.h, ctypes.byref(abi.ColliderPoses(count, poses.ctypes.data))) == abi.INVALID
            unchanged("count differs from the shapes' count")
            assert s.place_colliders_device(dev, count) == abi.INVALID
            unchanged("count differs from the shapes' count")
        for k, q, v in ((2, 0, np.nan), (1, 11, np.inf), (0, 4, -np.inf)):
            t = poses.copy()
            t[2, 5] = np.nan                                                       # the last collider too: the smallest is named
            t[k, q] = v
            assert s.place_colliders(t) == abi.INVALID
            unchanged("pose of collider %d is not finite" % k)
        host = poses.copy()
        pad = _hip.DeviceBuffer(2 * 36 + 2, pad=1)                                 # ptr = allocation + 4: 4-byte aligned only
        short = _hip.DeviceBuffer(2 * 36 - 2)                                      # one double short of 12 * 3
        for ptr, why in ((host.ctypes.data, "not device memory"), (pad.ptr, "not 8-byte aligned"), (short.ptr, "allocation ends before")):
            assert s.place_colliders_device(ptr, 3) == abi.INVALID, why
            unchanged(why)
        assert s.place_colliders_device(dev, 3) == abi.SUCCESS, s.last_error()     # the context stays usable
        assert_placed(s, *ref.place(col, idf, shapes, poses, sc.orig, sc.dx, 1), "after the refusals")
        pad.close()
        short.close()
        dev.close()
    finally:
        s.close()


# ---- 4. a non-finite pose ------------------------------------------------------------------------------------------------------------------
def test_device_table_with_a_nan_skips_that_collider_alone():
    sc, p, ids, shapes, poses, col, idf, counters = cases.build("three_negate")
    bad = poses.copy()
    bad[1, 10] = np.nan
    want = ref.place(sc.collision, ids, shapes, bad, sc.orig, sc.dx, 1)
    assert want[2][1] == 0 and want[2][-1] == 1 and counters[1] > 0
    s = polystokes_amd.Solver(0)
    try:
        assert s.set_collider_shapes(shapes) == abi.SUCCESS
        s.upload(sc, p)
        assert s.upload_collider_ids(ids) == abi.SUCCESS
        dev = on_device(bad)
        assert s.place_colliders_device(dev, 3) == abi.SUCCESS, s.last_error()
        assert_placed(s, *want, "nan")
        dev.close()
    finally:
        s.close()


# ---- 5. lifetime ---------------------------------------------------------------------------------------------------------------------------
def test_an_upload_erases_and_a_second_call_unions():
    case = "three_orig"                                                            # no id field: the call creates one
    sc, p, ids, shapes, poses, col, idf, counters = cases.build(case)
    s = polystokes_amd.Solver(0)
    try:
        cases.upload_and_place(s, case)
        assert_placed(s, col, idf, counters, "first")
        # the same poses: the same values and ids
        assert s.place_colliders(poses) == abi.SUCCESS
        c2, i2, n2 = ref.place(col, idf, shapes, poses, sc.orig, sc.dx, 1)
        assert_placed(s, c2, i2, n2, "again")
        assert np.array_equal(c2.view(np.uint32), col.view(np.uint32)) and np.array_equal(i2, idf)
        # other poses: a union on top of the first
        moved = poses.copy()
        moved[:, 9:] += (0.1, -0.05, 0.05)
        assert s.place_colliders(moved) == abi.SUCCESS
        c3, i3, n3 = ref.place(c2, i2, shapes, moved, sc.orig, sc.dx, 1)
        assert_placed(s, c3, i3, n3, "union")
        assert not np.array_equal(c3, c2) and (-c3.astype(np.float64) >= -c2.astype(np.float64)).all()
        # ids uploaded after a call replace the whole id field and do not re-place
        mod3 = cases.motions_cases.ids_field(sc, "mod3")
        assert s.upload_collider_ids(mod3) == abi.SUCCESS
        assert_placed(s, c3, mod3, n3, "ids after the call")
        assert s.upload_collider_ids(None) == abi.SUCCESS
        with pytest.raises(KeyError):
            s.array("colliderCellIds")
        assert s.array("collisionField").tobytes() == c3.tobytes()
        # an upload erases the arrays and the created id field, and restores the uploaded collision; the shapes stay
        s.upload(sc, p)
        for n in cases.ARRAYS:
            with pytest.raises(KeyError):
                s.array(n)
        assert int(s.array("colliderShapes")[0]) == 3
        assert s.place_colliders(poses) == abi.SUCCESS
        assert_placed(s, col, idf, counters, "after the upload")
    finally:
        s.close()


def test_picard_passes_keep_the_placement():
    sc, p, shapes, poses, motions = cases.step_scene()
    col, idf, counters = ref.place(sc.collision, None, shapes, poses, (0.0, 0.0, 0.0), sc.dx, 1)
    outcomes = []
    for placed_upload in (False, True):
        s = polystokes_amd.Solver(0)
        try:
            assert s.set_rheology(flow_index=0.7, passes=1, min_shear_rate=1e-2, min_viscosity=1e-3, max_viscosity=1e5) == abi.SUCCESS
            if placed_upload:
                sc2, p2 = cases.step_scene()[:2]
                sc2.collision = col.copy()
                s.upload(sc2, p2)
                assert s.upload_collider_ids(idf) == abi.SUCCESS
            else:
                assert s.set_collider_shapes(shapes) == abi.SUCCESS
                s.upload(sc, p)
                assert s.place_colliders(poses) == abi.SUCCESS
            outcomes.append(cases.step_outcome(s))
            assert len(s.array("rheologyIterations")) == 2
            if not placed_upload:
                assert_placed(s, col, idf, counters, "after the passes")
        finally:
            s.close()
    assert outcomes[0][0] == abi.SUCCESS and outcomes[0] == outcomes[1]


KEPT = {    # every array of the four features whose arrays outlive a setup, solve or step (ps_context::registerKeptArrays)
    "pockets": ("airPockets", "airPocketPasses", "airPocketIds", "airPocketUnits", "airPocketCells", "airPocketOpen", "airPocketVolume"),
    "motions": ("colliderMotions", "colliderMotionTable", "colliderMotionFaces", "collisionVelocityX", "collisionVelocityY", "collisionVelocityZ"),
    "shapes": ("colliderShapes",),
    "placement": ("colliderPlacement", "colliderPoseTable", "colliderPlacedCells", "collisionField", "colliderCellIds"),
}
TABLES = ("colliderMotions", "colliderMotionTable", "colliderMotionFaces", "colliderShapes", "colliderPlacement", "colliderPoseTable",
          "colliderPlacedCells")


def test_setup_solve_and_step_keep_the_four_features_arrays_and_an_upload_leaves_the_shapes():
    """Every name of the four lists answers ps_query_array after a setup, a solve, a step and a step with a Picard pass, the tables and
    counters byte for byte what the calls left; after the next upload "colliderShapes" alone is left."""
    sc, p = scenes.spheres(24, tile=8, nspheres=1)
    p.preconditioner = abi.PRE_DIAGONAL
    shape = cases.sphere_volume(0.09, 12, 1.0 / 44.0)
    centre = np.array([0.3, 0.3, 0.7])
    poses = cases.pose(shape, cases.rotation(np.random.RandomState(2)), centre).reshape(1, 12)
    motions = np.concatenate([(1.0, 0.0, 0.5), (0.0, 2.0, 0.0), centre]).reshape(1, 9)
    names = [n for group in KEPT.values() for n in group]
    assert len(names) == len(set(names)) == 19 and set(TABLES) <= set(names)
    s = polystokes_amd.Solver(0)
    try:
        def present():
            return {n: int(s.L.ps_query_array(s.h, n.encode(), None)) >= 0 for n in names}
        assert s.set_collider_shapes([shape]) == abi.SUCCESS
        s.upload(sc, p)
        assert s.place_colliders(poses) == abi.SUCCESS, s.last_error()
        assert s.upload_collider_ids(np.zeros((24, 24, 24), np.int32)) == abi.SUCCESS
        assert s.paint_collider_velocities(motions) == abi.SUCCESS, s.last_error()
        s.label_air_pockets()                                                      # (after the placement, which drops the labels)
        assert int(s.array("colliderPlacedCells")[0]) > 50 and int(s.array("colliderMotionFaces")[0]) > 0
        assert s.array("colliderPoseTable").tobytes() == poses.tobytes() and s.array("colliderMotionTable").tobytes() == motions.tobytes()
        before = {n: s.array(n).tobytes() for n in TABLES}

        def kept(stage):
            got = present()
            assert all(got.values()), (stage, [n for n in names if not got[n]])
            assert {n: s.array(n).tobytes() for n in TABLES} == before, stage
        kept("the calls")
        assert s.setup() == abi.SUCCESS
        kept("setup")
        s.solve()
        kept("solve")
        s.step_device()
        kept("step")
        assert s.set_rheology(flow_index=0.7, passes=1, min_shear_rate=1e-2, min_viscosity=1e-3, max_viscosity=1e5) == abi.SUCCESS
        s.step_device()
        assert len(s.array("rheologyIterations")) == 2                             # the pass ran
        kept("step with a Picard pass")
        s.upload(sc, p)
        got = present()
        assert [n for n in names if got[n]] == ["colliderShapes"], got
    finally:
        s.close()


def test_a_placement_drops_air_pocket_labels():
    sc, p, shapes, poses, motions = cases.step_scene()
    s = polystokes_amd.Solver(0)
    try:
        assert s.set_collider_shapes(shapes) == abi.SUCCESS
        s.upload(sc, p)
        s.label_air_pockets()
        assert s.array("airPockets") is not None
        dev = on_device(poses)
        assert s.place_colliders_device(dev, 2) == abi.SUCCESS, s.last_error()
        with pytest.raises(KeyError):
            s.array("airPockets")
        assert s.memory_stats()["deferred_bytes"] == 0
        s.label_air_pockets()                                                      # ... and the labels of the new solids can be made
        assert s.place_colliders_device(dev, 3) == abi.INVALID                     # a refusal keeps them
        assert s.array("airPockets") is not None
        dev.close()
    finally:
        s.close()


# ---- 6. memory -----------------------------------------------------------------------------------------------------------------------------
def test_memory_is_what_the_header_says_and_flat():
    case = "three_orig"                                                            # no id field: the call creates one
    sc, p, ids, shapes, poses, col, idf, counters = cases.build(case)
    samples = sum(int(np.prod(v.shape)) for v, _, _ in shapes)
    s = polystokes_amd.Solver(0)
    try:
        base0 = s.memory_stats()["live_bytes"]
        assert s.set_collider_shapes(shapes) == abi.SUCCESS
        mem = s.memory_stats()
        assert mem["deferred_bytes"] == 0 and mem["live_bytes"] - base0 == 4 * samples + 56 * 3      # include/polystokes.h
        s.upload(sc, p)
        base = s.memory_stats()["live_bytes"]
        assert s.place_colliders(poses) == abi.SUCCESS
        mem = s.memory_stats()
        assert mem["deferred_bytes"] == 0
        assert mem["live_bytes"] - base == 96 * 3 + 4 * 5 + 4 * sc.nx * sc.ny * sc.nz                 # the table, the counters, the created ids
        seen = []
        for _ in range(5):
            s.upload(sc, p)
            assert s.place_colliders(poses) == abi.SUCCESS
            assert s.memory_stats()["deferred_bytes"] == 0
            assert s.place_colliders(poses) == abi.SUCCESS
            mem = s.memory_stats()
            assert mem["deferred_bytes"] == 0
            seen.append(mem["live_bytes"])
        assert len(set(seen)) == 1 and seen[0] == base + 96 * 3 + 4 * 5 + 4 * sc.nx * sc.ny * sc.nz, seen
        assert s.set_collider_shapes(shapes[:2]) == abi.SUCCESS                    # other shapes: the previous pool goes
        assert s.memory_stats()["deferred_bytes"] == 0
        s.upload(sc, p)                                                            # the placement's buffers and the created ids go
        assert s.set_collider_shapes(None) == abi.SUCCESS
        mem = s.memory_stats()
        assert mem["deferred_bytes"] == 0 and mem["live_bytes"] == base - (4 * samples + 56 * 3)      # (base held the three volumes)
    finally:
        s.close()


# ---- 7. the loop closes ----------------------------------------------------------------------------------------------------------------------
def test_the_liquid_resists_a_placed_sphere_and_the_solid_follows_its_pose():
    """Signs only.  A sphere volume is placed in a pool at rest and painted with a velocity v: after one step the force of the liquid on
    it opposes v.  Moving its pose by one cell along v moves the centroid of the cells the setup finds mostly solid along v."""
    sc, p = scenes.spheres(32, tile=8, nspheres=1)
    p.preconditioner = abi.PRE_DIAGONAL
    for a in range(3):
        sc.vel[a][...] = 0.0
        sc.collisionvel[a][...] = 0.0
    other = np.array(cases.loads_cases.sphere_table(1)[0][0], np.float64)
    spots = [np.array(q) for q in ((0.3, 0.3, 0.3), (0.7, 0.3, 0.7), (0.3, 0.3, 0.7), (0.7, 0.3, 0.3))]
    centre = max(spots, key=lambda q: float(np.linalg.norm(q - other)))
    shape = cases.sphere_volume(0.09, 12, 1.0 / 44.0)
    rng = np.random.RandomState(2)
    R = cases.rotation(rng)
    v = np.array([1.0, 0.0, 0.0])
    tab = np.concatenate([v, np.zeros(3), centre]).reshape(1, 9)
    centroids = []
    s = polystokes_amd.Solver(0)
    try:
        assert s.set_collider_shapes([shape]) == abi.SUCCESS
        assert s.set_collider_loads(1, centre.reshape(1, 3)) == abi.SUCCESS
        for shift in (0.0, sc.dx):
            s.upload(sc, p)
            assert s.place_colliders(cases.pose(shape, R, centre + shift * v).reshape(1, 12)) == abi.SUCCESS, s.last_error()
            assert s.paint_collider_velocities(tab) == abi.SUCCESS
            assert s.step_device() == abi.SUCCESS
            if shift == 0.0:
                F = s.collider_loads()[0, 0:3]
                print("force", F.tolist(), "F.v", float(F @ v), "terms", s.array("colliderLoadTerms").tolist())
                assert float(F @ v) < 0
            fw = s.array("centerFluidWeights").reshape(sc.nz, sc.ny, sc.nx)
            mine = (fw < 0.5) & (s.array("colliderCellIds").reshape(fw.shape) == 0)
            assert mine.sum() > 30
            centroids.append(np.argwhere(mine).mean(axis=0)[::-1] @ v)            # (k, j, i) -> (x, y, z), in cells
        print("centroid along v, in cells", centroids)
        assert centroids[1] - centroids[0] > 0
    finally:
        s.close()

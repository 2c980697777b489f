"""Collider motions (ps_paint_collider_velocities) on the GPU.  The painted grids and the counters are a function of the upload — collision SDF,
ids, orig, dx — and the table, restated in numpy (collider_motions_ref.py): the device is compared with the restatement byte for byte, and a
step after a paint with a step of a fresh context uploaded with the restatement's grids.  test_collider_motions_ref_cpu.py shows that the
shared cases tell the rule from its near misses."""
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
import collider_loads_ref as loads_ref  # noqa: E402
import collider_motions_cases as cases  # noqa: E402
import collider_motions_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


def bits(g):
    return [np.ascontiguousarray(v).view(np.uint32) for v in g]


def assert_painted(s, grids, counters, what=""):
    g, n = cases.painted(s)
    print(what, "faces device", n.tolist(), "reference", np.asarray(counters).tolist())
    assert np.array_equal(n, counters), what
    for a in range(3):
        bad = np.argwhere(bits(g)[a] != bits(grids)[a])
        assert bad.size == 0, (what, a, len(bad), bad[:4].tolist())


def table_on_device(tab):
    return _hip.DeviceBuffer.from_numpy(np.ascontiguousarray(tab, np.float64).view(np.float32))


_fresh = {}


def fresh_outcome(case):
    """the step of a fresh context uploaded with the restatement's grids as collisionvel; computed once"""
    if case not in _fresh:
        sc2, p = cases.painted_scene(case)
        s = polystokes_amd.Solver(0)
        try:
            s.upload(sc2, p)
            _fresh[case] = cases.step_outcome(s)
        finally:
            s.close()
    return _fresh[case]


# ---- 1. against the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(cases.CASES))
def test_paint_equals_the_restatement(case):
    sc, p, ids, tab, grids, counters = cases.build(case)
    s = polystokes_amd.Solver(0)
    try:
        cases.upload_and_paint(s, case)                                            # host ids, host table
        assert int(s.array("colliderMotions")[0]) == tab.shape[0]
        assert s.array("colliderMotionTable").tobytes() == tab.tobytes()
        assert_painted(s, grids, counters, "host")
        # ids from device memory in z-fastest layout, the table from device memory
        s.upload(sc, p)
        dev_ids = None
        if ids is not None:
            dev_ids = _hip.DeviceBuffer.from_numpy(np.ascontiguousarray(ids.transpose(2, 1, 0)).view(np.float32))
            assert s.upload_collider_ids_device(dev_ids, abi.LAYOUT_Z_FASTEST) == abi.SUCCESS, s.last_error()
        dev_tab = table_on_device(tab)
        assert s.paint_collider_velocities_device(dev_tab, tab.shape[0]) == abi.SUCCESS, s.last_error()
        assert_painted(s, grids, counters, "device")
        dev_tab.close()
        if dev_ids is not None:
            dev_ids.close()
    finally:
        s.close()


@pytest.mark.parametrize("case,cap", [("spheres_nearest", 2), ("box_count64", 1), ("blob_mod3_both", 3)])
def test_a_workgroup_that_walks_several_tiles_paints_the_same(case, cap, monkeypatch):
    """The launch caps its workgroups per face grid at 2048 and strides the rest: grids of these sizes never get there.
    PS_DEBUG_MOTION_GRID lowers the cap (lab build), so that every workgroup walks many tiles, the last one ragged."""
    sc, p, ids, tab, grids, counters = cases.build(case)
    assert sc.nx * sc.ny * (sc.nz + 1) > 2 * 1024 * cap                            # more than two tiles of 256 x 4 faces per workgroup
    monkeypatch.setenv("PS_DEBUG_MOTION_GRID", str(cap))
    s = polystokes_amd.Solver(0)
    try:
        cases.upload_and_paint(s, case)
        assert_painted(s, grids, counters, "cap %d" % cap)
    finally:
        s.close()


# ---- 2. / 3. a step after painting ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.STEP_CASES)
def test_step_after_paint_equals_a_step_of_the_painted_upload(case):
    sc, p, ids, tab, grids, counters = cases.build(case)
    s = polystokes_amd.Solver(0)
    try:
        cases.upload_and_paint(s, case)
        got = cases.step_outcome(s)
        want = fresh_outcome(case)
        assert got[0] == abi.SUCCESS and got[:3] == want[:3], (got[:3], want[:3])
        assert got[3] == want[3] and got[4] == want[4]
        assert_painted(s, grids, counters, "after the step")                       # the step kept the arrays and the buffers
        # 3. every output face labelled SOLID holds the painted value
        solid = 0
        for a, name in enumerate(("faceXLabels", "faceYLabels", "faceZLabels")):
            lab = s.array(name).reshape(grids[a].shape)
            at = lab == abi.SOLID
            solid += int(at.sum())
            assert np.array_equal(s.vel[a].view(np.uint32)[at], grids[a].view(np.uint32)[at]), a
        print("SOLID faces", solid)
        assert solid > 100
    finally:
        s.close()


# ---- 4. a non-finite motion ----------------------------------------------------------------------------------------------------------------
def test_device_table_with_a_nan_leaves_that_collider_alone():
    case = "spheres_nearest"
    sc, p, ids, tab, grids, counters = cases.build(case)
    bad = tab.copy()
    bad[3, 4] = np.nan                                                             # w[1] of collider 3
    want_g, want_n = ref.paint(sc.collision, ids, bad, sc.orig, sc.dx, 1, sc.collisionvel)
    assert want_n[-1] == counters[3] > 0 and want_n[3] == 0
    s = polystokes_amd.Solver(0)
    try:
        s.upload(sc, p)
        assert s.upload_collider_ids(ids) == abi.SUCCESS
        dev = table_on_device(bad)
        assert s.paint_collider_velocities_device(dev, 8) == abi.SUCCESS, s.last_error()
        assert_painted(s, want_g, want_n, "nan")
        g, _ = cases.painted(s)
        for a in range(3):
            chosen, _ = ref.chosen_cells(sc.collision, a)
            three = ids[chosen] == 3
            assert np.array_equal(g[a][three], sc.collisionvel[a][three])          # untouched
            assert np.array_equal(g[a][~three].view(np.uint32), grids[a][~three].view(np.uint32))   # all others as before
        dev.close()
    finally:
        s.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    case = "blob_mod3_both"
    sc, p, ids, tab, grids, counters = cases.build(case)
    s = polystokes_amd.Solver(0)
    try:
        assert s.paint_collider_velocities(tab) == abi.INVALID and "call ps_upload_fields first" in s.last_error()
        dev = table_on_device(tab)
        assert s.paint_collider_velocities_device(dev, 3) == abi.INVALID and "call ps_upload_fields first" in s.last_error()
        cases.upload_and_paint(s, case)
        before = [s.array(n).tobytes() for n in cases.ARRAYS]

        def unchanged(why):
            assert why in s.last_error(), (why, s.last_error())
            assert [s.array(n).tobytes() for n in cases.ARRAYS] == before, why
        assert s.L.ps_paint_collider_velocities(s.h, None) == abi.INVALID
        unchanged("motions is null")
        assert s.L.ps_paint_collider_velocities(s.h, ctypes.byref(abi.ColliderMotions(3, None))) == abi.INVALID
        unchanged("motion is null")
        assert s.paint_collider_velocities_device(None, 3) == abi.INVALID
        unchanged("motion is null")
        for count in (0, -1, 65):
            assert s.L.ps_paint_collider_velocities(s.h, ctypes.byref(abi.ColliderMotions(count, tab.ctypes.data))) == abi.INVALID
            unchanged("count outside 1..64")
            assert s.paint_collider_velocities_device(dev, count) == abi.INVALID
            unchanged("count outside 1..64")
        for k, q, v in ((2, 0, np.nan), (1, 8, np.inf), (0, 4, -np.inf)):
            t = tab.copy()
            t[2, 5] = np.nan                                                       # the last collider too: the smallest is named
            t[k, q] = v
            assert s.paint_collider_velocities(t) == abi.INVALID
            unchanged("motion of collider %d is not finite" % k)
        # the pointer refusals of the device form
        host = tab.copy()
        pad = _hip.DeviceBuffer(2 * 27 + 2, pad=1)                                 # ptr = allocation + 4: 4-byte aligned only
        short = _hip.DeviceBuffer(2 * 27 - 2)                                      # one double short of 9 * 3
        for ptr, why in ((host.ctypes.data, "not device memory"), (pad.ptr, "not 8-byte aligned"), (short.ptr, "allocation ends before")):
            assert s.paint_collider_velocities_device(ptr, 3) == abi.INVALID, why
            unchanged(why)
        assert s.paint_collider_velocities_device(short, 2) == abi.SUCCESS, s.last_error()   # long enough for two
        pad.close()
        short.close()
        dev.close()
    finally:
        s.close()


# ---- 6. lifetime ---------------------------------------------------------------------------------------------------------------------------
def test_an_upload_erases_and_a_second_paint_paints_over():
    case = "box_rotation"                                                          # id 2 lies outside the count: those faces keep what they hold
    sc, p, ids, tab, grids, counters = cases.build(case)
    s = polystokes_amd.Solver(0)
    try:
        cases.upload_and_paint(s, case)
        assert_painted(s, grids, counters, "first")
        second = cases.table("both", 2, seed=23)
        assert s.paint_collider_velocities(second) == abi.SUCCESS
        over_g, over_n = ref.paint(sc.collision, ids, second, sc.orig, sc.dx, 1, grids)     # over the first paint
        assert_painted(s, over_g, over_n, "second")
        assert np.array_equal(over_n, counters) and any(not np.array_equal(over_g[a], grids[a]) for a in range(3))
        # ids uploaded after a paint do not repaint
        assert s.upload_collider_ids(np.zeros_like(ids)) == abi.SUCCESS
        assert_painted(s, over_g, over_n, "ids after the paint")
        # an upload erases the arrays and restores the uploaded collisionvel: a paint of everything-outside leaves it alone and shows it
        s.upload(sc, p)
        for n in cases.ARRAYS:
            with pytest.raises(KeyError):
                s.array(n)
        assert s.upload_collider_ids(np.full_like(ids, 5)) == abi.SUCCESS
        assert s.paint_collider_velocities(second) == abi.SUCCESS
        g, n = cases.painted(s)
        assert n.tolist() == [0, 0, int(counters.sum()), 0]
        for a in range(3):
            assert np.array_equal(g[a], sc.collisionvel[a])
    finally:
        s.close()


def test_picard_passes_keep_the_paint():
    case = "blob_mod3_both"
    sc, p, ids, tab, grids, counters = cases.build(case)
    outcomes = []
    for painted_upload in (False, True):
        s = polystokes_amd.Solver(0)
        try:
            assert s.set_rheology(flow_index=0.7, passes=1, min_shear_rate=1e-2, min_viscosity=1e-3, max_viscosity=1e5) == abi.SUCCESS
            if painted_upload:
                sc2, p2 = cases.painted_scene(case)
                s.upload(sc2, p2)
            else:
                cases.upload_and_paint(s, case)
            outcomes.append(cases.step_outcome(s))
            assert len(s.array("rheologyIterations")) == 2
            if not painted_upload:
                assert_painted(s, grids, counters, "after the passes")
        finally:
            s.close()
    assert outcomes[0][0] == abi.SUCCESS and outcomes[0] == outcomes[1]


# ---- 7. poison -----------------------------------------------------------------------------------------------------------------------------
def test_poisoned_buffers_change_nothing():
    """PS_DEBUG_POISON=1 fills whatever a buffer allocation hands out with 0xff: a kernel that read a word nobody wrote would show"""
    case = "spheres_nearest"
    sc, p, ids, tab, grids, counters = cases.build(case)
    pr = children.run_script("collider_motions_cases.py", "paint", case, limit=600, env={"PS_DEBUG_POISON": "1"}, drop=("PS_LIB",),
                             expect=("PS_DEBUG_POISON=1 is active",))              # the child read the switch
    assert pr.digests() == [(cases.digest(grids + [counters]), cases.outcome_digest(fresh_outcome(case)))], pr.output[-2000:]


# ---- 8. memory -----------------------------------------------------------------------------------------------------------------------------
def test_memory_is_flat_and_nothing_waits_for_release():
    case = "blob_mod3_both"
    sc, p, ids, tab, grids, counters = cases.build(case)
    count = tab.shape[0]
    s = polystokes_amd.Solver(0)
    try:
        s.upload(sc, p)
        assert s.upload_collider_ids(ids) == abi.SUCCESS
        base = s.memory_stats()["live_bytes"]
        assert s.paint_collider_velocities(tab) == abi.SUCCESS
        mem = s.memory_stats()
        assert mem["deferred_bytes"] == 0
        assert mem["live_bytes"] - base == 72 * count + 4 * (count + 2)            # include/polystokes.h
        assert s.paint_collider_velocities(tab[:2]) == abi.SUCCESS                 # another count: the previous pair goes
        mem = s.memory_stats()
        assert mem["deferred_bytes"] == 0 and mem["live_bytes"] - base == 72 * 2 + 4 * 4
        seen = []
        for _ in range(5):
            cases.upload_and_paint(s, case)
            assert s.memory_stats()["deferred_bytes"] == 0
            assert s.step_device() == abi.SUCCESS
            mem = s.memory_stats()
            assert mem["deferred_bytes"] == 0
            seen.append(mem["live_bytes"])
        assert len(set(seen)) == 1, seen
    finally:
        s.close()


# ---- 9. the loop closes ----------------------------------------------------------------------------------------------------------------------
def test_the_liquid_resists_a_spinning_sphere():
    """One sphere in a pool at rest spins about its own centre.  The torque of the liquid on it, about that centre, opposes the spin:
    T . w < 0, by ten times the loads' own bound (terms + 8) 2^-53 B |w| at the least."""
    sc, p = scenes.spheres(32, tile=8, nspheres=1)
    p.preconditioner = abi.PRE_DIAGONAL
    for a in range(3):
        sc.vel[a][...] = 0.0
    centre = np.array(cases.loads_cases.sphere_table(1)[0][0], np.float64)
    w = np.array([0.0, 0.0, 5.0])
    tab = np.concatenate([np.zeros(3), w, centre]).reshape(1, 9)
    s = polystokes_amd.Solver(0)
    try:
        s.upload(sc, p)
        assert s.set_collider_loads(1, centre.reshape(1, 3)) == abi.SUCCESS
        assert s.paint_collider_velocities(tab) == abi.SUCCESS                     # no id field: collider 0 everywhere
        want_g, want_n = ref.paint(sc.collision, None, tab, (0.0, 0.0, 0.0), sc.dx, 1, sc.collisionvel)
        assert_painted(s, want_g, want_n, "spin")
        assert s.step_device() == abi.SUCCESS
        T = s.collider_loads()[0, 3:6]
        terms = s.array("colliderLoadTerms")
        B = s.array("colliderLoadScale").reshape(1, 6)[:, 3:]
        bound = float((loads_ref.bound(terms[:-1], B)[0] * np.abs(w)).sum())
        power = float(T @ w)
        print("torque", T.tolist(), "T.w", power, "bound", bound, "terms", terms.tolist())
        assert power < 0
        assert abs(power) > 10.0 * bound
    finally:
        s.close()

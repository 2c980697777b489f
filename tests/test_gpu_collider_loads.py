"""Collider loads (ps_set_collider_loads) on the GPU.  The loads are a function of the step's own arrays — weights, index maps, x — restated
in numpy (collider_loads_ref.py): every comparison feeds the restatement what the step left (its weight arrays and solution_fields()) and
asks for  |F - F_ref| <= (terms_k + 8) 2^-53 A_k  per axis, the same with B_k for the torque and for the scales themselves, and equal
counts.  test_collider_loads_ref_cpu.py shows that these scenes tell the rule from its near misses and fixes sign and scale."""
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
import collider_loads_cases as cases  # noqa: E402
import collider_loads_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

# scene, id field, count, pivots
CASES = {
    "blob_no_ids": ("blob", None, 1, None),
    "spheres_nearest": ("spheres32", "spheres", 8, "spheres"),
    "spheres_mod3": ("spheres32", "mod3", 3, "diagonal"),
    "sliding_two": ("sliding32", None, 2, "diagonal"),
}


def check(s, sc, count, ids=None, pivots=None):
    """the step's arrays against the restatement; returns (got, want)"""
    assert int(s.array("colliderLoads")[0]) == count
    g, w = cases.got(s), cases.want(s, sc, count, ids, pivots)
    for name, a, b in zip("F T n A B".split(), g, w):
        print(name, "device", np.asarray(a).tolist(), "reference", np.asarray(b).tolist())
    print("bound F", ref.bound(w[2][:-1], w[3]).tolist(), "bound T", ref.bound(w[2][:-1], w[4]).tolist())
    assert ref.outside(g, w) == []
    return g, w


def getters(s, count):
    """(host getter, device getter) as (count, 6) arrays"""
    host = s.collider_loads()
    buf = _hip.DeviceBuffer(12 * count)
    assert s.collider_loads_device(buf, 6 * count) == abi.SUCCESS, s.last_error()
    dev = buf.to_numpy().view(np.float64).reshape(count, 6)       # (a blocking copy on the default stream: it follows the getter's)
    buf.close()
    return host, dev


# ---- 1. against the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_step_equals_the_restatement(case):
    name, kind, count, pk = CASES[case]
    sc, p = cases.scene(name)
    ids, piv = cases.ids_field(sc, kind), cases.pivots_for(sc, count, pk)
    s = polystokes_amd.Solver(0)
    try:
        assert cases.step(s, sc, p, count, ids, piv) == abi.SUCCESS
        g, w = check(s, sc, count, ids, piv)
        n = w[2]
        assert int(n[:-1].sum()) > 100                                             # the case is not vacuous
        if case == "spheres_nearest":
            assert n[8] > 0 and np.all(n[:8] > 0), n                               # eight colliders, and dropped terms
        if case == "spheres_mod3":
            assert np.all(n[:3] > 0) and n[3] == 0, n
        if case == "sliding_two":
            assert n[1] == 0 and not g[0][1].any() and not g[1][1].any()           # a collider nobody names: zeros
        # host getter = device getter = arrays, bit for bit
        host, dev = getters(s, count)
        both = np.concatenate([g[0], g[1]], axis=1)
        assert host.tobytes() == dev.tobytes() == both.tobytes()
    finally:
        s.close()


def test_null_pivots_are_the_origin_of_the_upload():
    sc, p = cases.scene("blob")
    sc.orig = (0.375, -1.25, 2.5)
    s = polystokes_amd.Solver(0)
    try:
        assert cases.step(s, sc, p, 2, None, None) == abi.SUCCESS
        a, _ = check(s, sc, 2)                                                     # (the restatement's default pivot is the scene's orig)
        assert cases.step(s, sc, p, 2, None, [sc.orig, sc.orig]) == abi.SUCCESS
        b = cases.got(s)
        assert cases.digest(a) == cases.digest(b)
        assert cases.step(s, sc, p, 2, None, [[0.0, 0.0, 0.0], sc.orig]) == abi.SUCCESS
        c, _ = check(s, sc, 2, None, [[0.0, 0.0, 0.0], sc.orig])
        assert c[0].tobytes() == a[0].tobytes() and c[1].tobytes() != a[1].tobytes()   # the force does not see the pivot, the torque does
    finally:
        s.close()


# ---- 2. reproducible ---------------------------------------------------------------------------------------------------------------------
def _digest_of(case, s=None):
    name, kind, count, pk = CASES[case]
    sc, p = cases.scene(name)
    own = s is None
    s = polystokes_amd.Solver(0) if own else s
    try:
        assert cases.step(s, sc, p, count, cases.ids_field(sc, kind), cases.pivots_for(sc, count, pk)) == abi.SUCCESS
        return cases.digest(cases.got(s)), cases.digest([s.collider_loads()])
    finally:
        if own:
            s.close()


@pytest.mark.parametrize("case", ["spheres_nearest", "spheres_mod3"])
def test_bitwise_equal_across_runs_and_contexts(case):
    s = polystokes_amd.Solver(0)
    try:
        first, second = _digest_of(case, s), _digest_of(case, s)
    finally:
        s.close()
    assert first == second == _digest_of(case)


def test_poisoned_buffers_change_nothing():
    """PS_DEBUG_POISON=1 fills whatever a buffer allocation hands out with 0xff: a sum that read a partial nobody wrote would show"""
    pr = children.run_script("collider_loads_cases.py", "step", "spheres32", "spheres", 8, limit=600, env={"PS_DEBUG_POISON": "1"}, drop=("PS_LIB",),
                             expect=("PS_DEBUG_POISON=1 is active",))              # the child read the switch
    assert pr.digests() == [_digest_of("spheres_nearest")], pr.output[-2000:]


def test_device_id_upload_equals_the_host_upload_in_both_layouts():
    name, kind, count, pk = CASES["spheres_nearest"]
    sc, p = cases.scene(name)
    ids, piv = cases.ids_field(sc, kind), cases.pivots_for(sc, count, pk)
    s = polystokes_amd.Solver(0)
    try:
        assert cases.step(s, sc, p, count, ids, piv) == abi.SUCCESS
        base = cases.digest(cases.got(s))
        for layout in (abi.LAYOUT_X_FASTEST, abi.LAYOUT_Z_FASTEST):
            flat = np.ascontiguousarray(ids if layout == abi.LAYOUT_X_FASTEST else ids.transpose(2, 1, 0))
            dev = _hip.DeviceBuffer.from_numpy(flat.view(np.float32))
            s.upload(sc, p)
            assert s.upload_collider_ids_device(dev, layout) == abi.SUCCESS, s.last_error()
            assert s.step_device() == abi.SUCCESS
            assert cases.digest(cases.got(s)) == base, layout
            dev.close()
        s.upload(sc, p)                                                            # an upload drops the ids: collider 0 takes every term
        assert s.step_device() == abi.SUCCESS
        n = s.array("colliderLoadTerms")
        assert n[0] > 0 and not n[1:].any(), n
    finally:
        s.close()


# ---- 3. off by default, and the loads only read ------------------------------------------------------------------------------------------
def _step_outcome(s, sc, p):
    rc = s.step_device()
    s.download()
    return (int(rc), int(s.stats.result), int(s.stats.solveData[1]), s.array("solutionVector").tobytes(),
            [v.tobytes() for v in s.vel], [v.tobytes() for v in s.valid])


def test_off_by_default_and_a_step_is_the_same_with_the_setting_on():
    name, kind, count, pk = CASES["spheres_nearest"]
    sc, p = cases.scene(name)
    plain = polystokes_amd.Solver(0)
    s = polystokes_amd.Solver(0)
    try:
        plain.upload(sc, p)
        base = _step_outcome(plain, sc, p)
        assert int(plain.array("colliderLoads")[0]) == 0
        for n in cases.RESULT_ARRAYS:
            with pytest.raises(KeyError):
                plain.array(n)
        with pytest.raises(polystokes_amd.PolyStokesError):
            plain.collider_loads()
        s.upload(sc, p)
        assert s.set_collider_loads(count, cases.pivots_for(sc, count, pk)) == abi.SUCCESS
        assert s.upload_collider_ids(cases.ids_field(sc, kind)) == abi.SUCCESS
        assert _step_outcome(s, sc, p) == base
        assert int(s.array("colliderLoads")[0]) == count
        assert s.set_collider_loads(0) == abi.SUCCESS                              # back to off: the arrays go, the step is the same
        for n in cases.RESULT_ARRAYS:
            with pytest.raises(KeyError):
                s.array(n)
        s.upload(sc, p)
        assert _step_outcome(s, sc, p) == base
        assert int(s.array("colliderLoads")[0]) == 0
    finally:
        plain.close()
        s.close()


# ---- 4. paths ----------------------------------------------------------------------------------------------------------------------------
def test_split_and_one_call_entry_points():
    sc, p = cases.scene("blob")
    s = polystokes_amd.Solver(0)
    try:
        assert s.set_collider_loads(1) == abi.SUCCESS
        s.upload(sc, p)                                                            # ps_setup_device + ps_solve_device
        s.setup()
        assert s.solve() == abi.SUCCESS
        a, _ = check(s, sc, 1)
        assert s.step(sc, p) == abi.SUCCESS                                        # polystokes_step
        b, _ = check(s, sc, 1)
        assert cases.digest(a) == cases.digest(b)
        for layout in (abi.LAYOUT_X_FASTEST, abi.LAYOUT_Z_FASTEST):                # ps_step_device_fields
            ds = polystokes_amd.device_scene(sc, layout)
            rc, _, _ = s.step_device_fields(p, ds, layout)
            assert rc == abi.SUCCESS, s.last_error()
            assert cases.digest(cases.got(s)) == cases.digest(a), layout
    finally:
        s.close()


@pytest.mark.parametrize("path", ["eigen", "mixed", "noconverge"])
def test_solver_paths(path):
    sc, p = cases.scene("spheres32")
    ids = cases.ids_field(sc, "mod3")
    s = polystokes_amd.Solver(0)
    try:
        want_rc = abi.SUCCESS
        if path == "eigen":
            p.solverType = abi.EIGEN
        elif path == "mixed":
            assert s.set_solve_precision(abi.PRECISION_MIXED) == abi.SUCCESS
        else:
            p.maxSolverIterations, p.keepNonConvergedResults, want_rc = 5, 1, abi.NOCONVERGE
        assert cases.step(s, sc, p, 3, ids) == want_rc
        if path == "mixed":
            assert int(s.array("solvePrecisionUsed")[0]) != 0
        _, w = check(s, sc, 3, ids)
        assert np.all(w[2][:3] > 0)
    finally:
        s.close()


def test_picard_passes_leave_the_last_pass():
    sc, p = cases.scene("blob")
    s = polystokes_amd.Solver(0)
    try:
        assert s.set_rheology(flow_index=0.7, passes=2, min_shear_rate=1e-2, min_viscosity=1e-3, max_viscosity=1e5) == abi.SUCCESS
        assert cases.step(s, sc, p, 1) == abi.SUCCESS
        assert len(s.array("rheologyIterations")) == 3
        check(s, sc, 1)                                                            # (solution_fields() is the last pass's x)
    finally:
        s.close()


def test_steps_that_compute_no_loads():
    sc, p = cases.scene("spheres32")
    s = polystokes_amd.Solver(0)

    def nothing():
        assert int(s.array("colliderLoads")[0]) == 0
        for n in cases.RESULT_ARRAYS:
            with pytest.raises(KeyError):
                s.array(n)
        with pytest.raises(polystokes_amd.PolyStokesError):
            s.collider_loads()
        assert "computed no loads" in s.last_error()
    try:
        long_p = cases.scene("spheres32")[1]
        long_p.tolerance, long_p.maxSolverIterations = 1e-8, 20000                 # a solve long enough to be interrupted
        s.upload(sc, long_p)
        assert s.set_collider_loads(3) == abi.SUCCESS
        s.set_interrupt(lambda: True)                                              # an interrupted step
        assert s.step_device() == abi.INCOMPLETE
        s.set_interrupt(None)
        nothing()
        p.maxSolverIterations, p.keepNonConvergedResults = 5, 0                    # a dropped NOCONVERGE
        s.upload(sc, p)
        assert s.step_device() == abi.NOCONVERGE
        nothing()
        sc2, p2 = cases.scene("spheres32")
        p2.doSolve = 0                                                             # a step that does not solve
        s.upload(sc2, p2)
        s.step_device()
        nothing()
        s.upload(sc2, cases.scene("spheres32")[1])                                 # and the next good step computes them again
        assert s.step_device() == abi.SUCCESS
        check(s, sc2, 3)
        s.upload(sc2, cases.scene("spheres32")[1])                                 # an upload forgets them
        with pytest.raises(polystokes_amd.PolyStokesError):
            s.collider_loads()
    finally:
        s.close()


def test_in_process_group_ignores_the_setting():
    sc, p = scenes.cavity(32, tile=8)
    runs = []
    for count in (None, 3):
        g = polystokes_amd.Group(2)
        try:
            if count is not None:
                assert g.set_collider_loads(count) == abi.SUCCESS
            rc = g.solve_scene(sc, p)
            for r in g.ranks:
                assert int(r.array("colliderLoads")[0]) == 0
                with pytest.raises(KeyError):
                    r.array("colliderForce")
            runs.append((rc, int(g.stats.solveData[1]), [v.tobytes() for v in g.vel], [v.tobytes() for v in g.valid]))
        finally:
            g.close()
    assert runs[0][0] == abi.SUCCESS and runs[0] == runs[1]


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    sc, p = cases.scene("blob")
    s = polystokes_amd.Solver(0)
    try:
        assert s.upload_collider_ids(np.zeros(4, np.int32)) == abi.INVALID         # ids before any upload
        assert "call ps_upload_fields first" in s.last_error()
        assert s.upload_collider_ids_device(None) == abi.INVALID
        assert s.set_collider_loads(2, [[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]]) == abi.SUCCESS
        assert s.set_collider_loads(65) == abi.INVALID and "count outside 0..64" in s.last_error()
        assert s.set_collider_loads(-1) == abi.INVALID and "count outside 0..64" in s.last_error()
        assert s.set_collider_loads(2, [[0.0, np.nan, 0.0], [1.0, 2.0, 3.0]]) == abi.INVALID and "pivot 0 is not finite" in s.last_error()
        assert s.set_collider_loads(2, [[0.0, 0.0, 0.0], [1.0, np.inf, 3.0]]) == abi.INVALID and "pivot 1 is not finite" in s.last_error()
        assert s.L.ps_set_collider_loads(s.h, None) == abi.INVALID
        s.upload(sc, p)
        assert s.step_device() == abi.SUCCESS
        check(s, sc, 2, None, [[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]])                  # the refused calls kept the setting
        out = np.zeros(12)
        assert s.L.ps_get_collider_loads(s.h, out.ctypes.data, 11) == abi.FAILED   # out_len short
        assert "fewer than 6 * count" in s.last_error() and not out.any()
        assert s.L.ps_get_collider_loads(s.h, out.ctypes.data, 12) == abi.SUCCESS
        # the pointer refusals of the _device calls
        nc = sc.nx * sc.ny * sc.nz
        good = _hip.DeviceBuffer(nc, pad=1)
        host = np.zeros(nc, np.int32)
        pinned = _hip.HostBuffer(nc)
        for ptr, layout, why in ((good, 2, "layout must be 0"), (host.ctypes.data, 0, "not device memory"), (pinned, 0, "not device memory"),
                                 (good.ptr + 2, 0, "not 4-byte aligned"), (good.ptr + 8, 0, "allocation ends before")):
            assert s.upload_collider_ids_device(ptr, layout) == abi.INVALID, why
            assert why in s.last_error(), (why, s.last_error())
        assert s.upload_collider_ids_device(good, 0) == abi.SUCCESS                 # (4-byte aligned only: a view with a storage offset)
        assert s.upload_collider_ids(None) == abi.SUCCESS
        for ptr, n, why in ((host.ctypes.data, 12, "not device memory"), (good.ptr, 12, "not 8-byte aligned"), (good.ptr + 4 + 4 * (nc - 22), 12, "allocation ends before")):
            assert s.collider_loads_device(ptr, n) == abi.INVALID, why
            assert why in s.last_error(), (why, s.last_error())
        with pytest.raises(polystokes_amd.PolyStokesError):
            s.collider_loads_device(good.ptr + 4, 11)
        pinned.close()
        good.close()
    finally:
        s.close()


# ---- 6. memory ---------------------------------------------------------------------------------------------------------------------------
def test_memory_is_flat_and_released_with_the_setting():
    sc, p = cases.scene("blob")
    count = 5
    s = polystokes_amd.Solver(0)
    try:
        s.upload(sc, p)
        s.step_device()
        s.step_device()
        base = s.memory_stats()["live_bytes"]
        assert s.set_collider_loads(count) == abi.SUCCESS
        assert s.memory_stats()["live_bytes"] == base                              # the setting alone allocates nothing
        seen = []
        for _ in range(5):
            assert s.step_device() == abi.SUCCESS and int(s.array("colliderLoads")[0]) == count
            mem = s.memory_stats()
            assert mem["deferred_bytes"] == 0
            seen.append(mem["live_bytes"])
        assert len(set(seen)) == 1, seen
        most = (sc.nx + 1) * (sc.ny + 1) * sc.nz                                   # the XY edge grid is the largest here (nz is the longest extent)
        assert most == max((sc.nx + 1) * (sc.ny + 1) * sc.nz, (sc.nx + 1) * sc.ny * (sc.nz + 1), sc.nx * (sc.ny + 1) * (sc.nz + 1))
        W = 4 * min(1024, -(-most // 256))
        assert seen[0] - base == W * (100 * count + 12) + 172 * count + 4, (seen[0] - base, W)     # include/polystokes.h
        ids = _hip.DeviceBuffer(sc.nx * sc.ny * sc.nz)
        assert s.upload_collider_ids_device(ids) == abi.SUCCESS
        assert s.memory_stats()["live_bytes"] == seen[0] + 4 * sc.nx * sc.ny * sc.nz               # one int32 cell grid while present
        assert s.upload_collider_ids(None) == abi.SUCCESS
        ids.close()
        assert s.set_collider_loads(0) == abi.SUCCESS
        mem = s.memory_stats()
        assert mem["deferred_bytes"] == 0 and mem["live_bytes"] == base
        with pytest.raises(KeyError):
            s.array("colliderForce")
    finally:
        s.close()


# ---- 7. physics --------------------------------------------------------------------------------------------------------------------------
def test_sliding_block_drags_the_floor_along():
    """The liquid box slides with u_x = U > 0 over a floor at rest.  The floor brakes it: the written velocity holds less x-momentum than
    the input (read off the downloaded fields, independently of the loads), so the reaction on the block opposes its velocity, -F_x U < 0,
    and the force on the solids is its opposite, along the block's velocity (Newton's third law; the sign the adjointness test of
    test_collider_loads_ref_cpu.py fixes from the recovery u = u* - dt McInv C x).  The size is far above the bound of the sums."""
    sc, p = cases.scene("sliding32")
    s = polystokes_amd.Solver(0)
    try:
        assert cases.step(s, sc, p, 1) == abi.SUCCESS
        s.download()
        g, w = check(s, sc, 1)
        ok = s.valid[0] > 0
        ok[:, :4, :] = False                                                       # liquid faces only: the floor's own faces take its velocity
        change = float((s.vel[0].astype(np.float64) - sc.vel[0])[ok].sum())
        U = float(sc.vel[0].max())
        print("x-velocity change summed over the valid faces", change, "F_x", g[0][0, 0], "bound", ref.bound(w[2][:-1], w[3])[0, 0])
        assert U > 0 and change < 0
        assert g[0][0, 0] > 1e6 * ref.bound(w[2][:-1], w[3])[0, 0]
        assert -g[0][0, 0] * U < 0
    finally:
        s.close()


def test_mirrored_scene_has_no_sideways_force():
    """A droplet falling on a floor, mirror-symmetric in x bit for bit: F_x = 0 in exact arithmetic.  The discretisation is not exactly
    symmetric (the oracle's cell labels of this scene are not mirror images), so the bound is what the issue sets: the item-4 bound plus
    ten times |F_x| of the oracle's fp64 solve of the same scene (measured: F_x = -0.0914 against A_x = 1.45 and |F_y| = 14.4)."""
    from oracle import ps_oracle
    sc, p = cases.mirrored_scene()
    o = ps_oracle.Oracle()
    assert o.run(sc, p) == abi.SUCCESS
    Fo = ref.loads(ref.inputs(o, sc, cases.oracle_solution(o, o.array("solutionVector"))), 1)[0]
    s = polystokes_amd.Solver(0)
    try:
        assert cases.step(s, sc, p, 1) == abi.SUCCESS
        g, w = check(s, sc, 1)
        bound = 10.0 * abs(Fo[0, 0]) + ref.bound(w[2][:-1], w[3])[0, 0]
        print("F device", g[0][0].tolist(), "F oracle", Fo[0].tolist(), "bound on |F_x|", bound)
        assert abs(g[0][0, 0]) <= bound
        assert abs(g[0][0, 1]) > 10 * bound                                        # the load it carries is the vertical one
    finally:
        s.close()

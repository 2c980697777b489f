"""Contact angles (ps_set_contact_angle, ps_upload_contact_cosine_field) on the GPU.

The oracle knows no surface tension, so every check is the numpy restatement of tests/contact_angle_ref.py (bit for bit for the rewritten
SDF), the existing restatements of the curvature and of the ghost-pressure impulse fed with it, or an ordering of the flow at the foot
of a hemisphere on a floor."""
import numpy as np
import pytest

import polystokes_amd
from polystokes_amd import _abi as abi
from polystokes_amd import _hip, scenes

import contact_angle_ref as ref
import surface_fields_ref as sref

pytestmark = pytest.mark.gpu

NEW_ARRAYS = ("contactCosine", "contactField", "contactCells", "surfaceWetted")


@pytest.fixture(scope="module")
def gpu():
    s = polystokes_amd.Solver(0)
    yield s
    s.close()


def _run(solver, sc, p):
    rc = solver.step(sc, p)
    assert rc == abi.SUCCESS, (rc, solver.last_error())
    return rc


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _absent(solver):
    for name in NEW_ARRAYS:
        with pytest.raises(KeyError):
            solver.array(name)
    assert float(solver.array("contactAngle")[0]) == -1.0


# ---- 1. the setting and the field --------------------------------------------------------------------------------------------------------
def test_setting_errors_and_persistence():
    s = polystokes_amd.Solver(0)
    try:
        sc, p = ref.hemisphere(sigma=1.0)
        assert s.set_contact_angle(60.0) == abi.SUCCESS
        for bad in (float("nan"), float("inf"), -float("inf"), 180.5, 1e300):
            assert s.set_contact_angle(bad) == abi.INVALID, bad
            assert "contact angle outside 0..180" in s.last_error()
        _run(s, sc, p)                                            # the refused calls kept 60; the setting survives the upload of the step
        assert float(s.array("contactAngle")[0]) == 60.0
        assert abs(float(s.array("contactCosine")[0]) - 0.5) <= 1e-15
        assert int(s.array("contactField")[0]) == 0 and int(s.array("contactCells")[0]) == 4 * 32 * 32
        for deg, cos in ((90.0, 0.0), (0.0, 1.0), (180.0, -1.0)):
            assert s.set_contact_angle(deg) == abi.SUCCESS
            _run(s, sc, p)
            assert float(s.array("contactAngle")[0]) == deg and float(s.array("contactCosine")[0]) == cos      # exactly
        assert s.set_contact_angle(-7.0) == abi.SUCCESS           # any negative value is off
        _run(s, sc, p)
        _absent(s)
    finally:
        s.close()


def test_field_errors_smallest_index_and_pointer_refusals():
    sc, p = scenes.blob(seed=4)
    sh = sc.surface.shape
    nc = sc.nx * sc.ny * sc.nz
    s = polystokes_amd.Solver(0)
    try:
        assert s.upload_contact_cosine_field(np.zeros(4, np.float32)) == abi.INVALID          # before any upload
        assert "call ps_upload_fields first" in s.last_error()
        assert s.upload_contact_cosine_field_device(None) == abi.INVALID
        sc.surface_tension = 0.5
        s.upload(sc, p)
        good = np.random.RandomState(1).uniform(-1, 1, sh).astype(np.float32)
        good[0, 0, 0], good[-1, -1, -1] = 1.0, -1.0                                             # the ends of the range are inside it
        assert s.upload_contact_cosine_field(good) == abi.SUCCESS
        # two bad values: (k, j, i) = (2, 17, 5) comes first in x-fastest numbering, (20, 1, 3) first in z-fastest storage
        first = (2 * sc.ny + 17) * sc.nx + 5
        for v_first, v_second in ((1.0000001, -2.0), (np.nan, 3.0), (-np.inf, np.nan)):
            f = good.copy()
            f[2, 17, 5], f[20, 1, 3] = v_first, v_second
            want = "contact cosine: value outside [-1, 1] at cell %d" % first
            assert s.upload_contact_cosine_field(f) == abi.INVALID
            assert want in s.last_error(), s.last_error()
            for layout in (abi.LAYOUT_X_FASTEST, abi.LAYOUT_Z_FASTEST):
                dev = _hip.DeviceBuffer.from_numpy(polystokes_amd.to_layout(f, layout), pad=1)
                assert s.upload_contact_cosine_field_device(dev, layout) == abi.INVALID
                assert want in s.last_error(), (layout, s.last_error())
                dev.close()
        assert s.step_device() == abi.SUCCESS                       # the refusals dropped the field, and the scalar is off
        _absent(s)
        # the pointer refusals of the _device calls
        ok = _hip.DeviceBuffer.from_numpy(good, pad=1)
        host = np.zeros(nc, np.float32)
        pinned = _hip.HostBuffer(nc)
        for ptr, layout, why in ((ok, 2, "layout must be 0"), (host.ctypes.data, 0, "not device memory"), (pinned, 0, "not device memory"),
                                 (ok.ptr + 2, 0, "not 4-byte aligned"), (ok.ptr + 8, 0, "allocation ends before")):
            assert s.upload_contact_cosine_field_device(ptr, layout) == abi.INVALID, why
            assert why in s.last_error(), (why, s.last_error())
        assert s.upload_contact_cosine_field_device(ok, 0) == abi.SUCCESS                       # (4-byte aligned only)
        assert s.step_device() == abi.SUCCESS
        assert int(s.array("contactField")[0]) == 1 and float(s.array("contactAngle")[0]) == -1.0   # the field alone turns the rule on
        s.upload(sc, p)                                              # every upload drops the field
        assert s.step_device() == abi.SUCCESS
        _absent(s)
        pinned.close()
        ok.close()
    finally:
        s.close()


# ---- 2. off is off ---------------------------------------------------------------------------------------------------------------------
def _outputs(s):
    return ([v.tobytes() for v in s.vel], [v.tobytes() for v in s.valid], s.array("b").tobytes(), int(s.stats.solveData[1]))


def test_off_is_off():
    sc, p = scenes.blob(seed=2)
    sc.vel[1][:] -= 0.3
    never, back, nosigma, never0 = (polystokes_amd.Solver(0) for _ in range(4))
    try:
        sc.surface_tension = 2.0
        _run(never, sc, p)                                          # never made the call
        assert back.set_contact_angle(60.0) == abi.SUCCESS
        _run(back, sc, p)
        assert int(back.array("contactCells")[0]) > 0
        assert _outputs(back) != _outputs(never)                    # (the angle does change this scene)
        assert back.set_contact_angle(-1.0) == abi.SUCCESS          # the angle set to -1 after having been 60
        _run(back, sc, p)
        assert _outputs(back) == _outputs(never)
        sc.surface_tension = 0.0
        _run(never0, sc, p)
        assert nosigma.set_contact_angle(60.0) == abi.SUCCESS       # the angle 60 but sigma = 0: no curvature, no rule
        _run(nosigma, sc, p)
        assert _outputs(nosigma) == _outputs(never0)
        for s in (never, back, nosigma, never0):
            _absent(s)
    finally:
        for s in (never, back, nosigma, never0):
            s.close()


# ---- 3. the rewritten SDF, bit for bit ---------------------------------------------------------------------------------------------------
def _crafted(kind):
    surface, collision, dx = ref.crafted_constant() if kind == "constant" else ref.crafted_ramp()
    nz, ny, nx = surface.shape
    sc = abi.Scene(nx, ny, nz, dx, 1.0 / 24.0, 1000.0, [0.0, 0.0, 0.0], surface, collision, 10.0, name="crafted_" + kind)
    return sc, abi.default_params(tileSize=8)


def _wetting_case(name):
    """(scene, params, scalar degrees or None, cosine field or None)"""
    if name.startswith("hemisphere"):
        sc, p = ref.hemisphere()
        return sc, p, float(name[len("hemisphere"):]), None
    if name in ("constant", "ramp"):
        sc, p = _crafted(name)
        return sc, p, 45.0, None
    sc, p = scenes.blob(21, 18, 27, seed=5) if name.startswith("odd") else scenes.blob(seed=2)
    field = None
    if name.endswith("field"):
        field = np.random.RandomState(11).uniform(-1, 1, sc.surface.shape).astype(np.float32)
    if name == "blob_negate0":
        sc.collision[:] = -sc.collision
        p.negateCollision = 0
    return sc, p, (None if name == "blob_field" else 70.0), field


@pytest.mark.parametrize("name", ["hemisphere60", "hemisphere90", "hemisphere120", "blob_scalar", "blob_field", "odd_scalar", "odd_both_field",
                                  "constant", "ramp", "blob_negate0"])
def test_wetted_sdf_bit_for_bit(name):
    sc, p, deg, field = _wetting_case(name)
    s = polystokes_amd.Solver(0)
    try:
        sc.surface_tension = 0.07
        assert s.set_contact_angle(-1.0 if deg is None else deg) == abi.SUCCESS
        s.upload(sc, p)
        if field is not None:
            assert s.upload_contact_cosine_field(field) == abi.SUCCESS
        s.step_device()                                            # (a crafted scene is all solid: its system is empty)
        cos = float(s.array("contactCosine")[0])
        assert float(s.array("contactAngle")[0]) == (-1.0 if deg is None else deg)
        assert int(s.array("contactField")[0]) == (0 if field is None else 1)
        got = s.array("surfaceWetted").reshape(sc.surface.shape)
        want = ref.wetted(sc.surface, sc.collision, sc.dx, cos if field is None else field, negate=int(p.negateCollision))
        U = ref.update_set(sc.collision, sc.dx, negate=int(p.negateCollision))
        assert int(s.array("contactCells")[0]) == int(U.sum()) and U.sum() > 0
        assert np.array_equal(_bits(got), _bits(want)), int((_bits(got) != _bits(want)).sum())
        if name == "constant":
            assert np.array_equal(_bits(got), _bits(sc.surface))
        else:
            assert (got != sc.surface).any()
        if name == "blob_negate0":                                # the flipped field with negateCollision = 0 is the same solid
            sc1, _, _, _ = _wetting_case("blob_scalar")
            assert np.array_equal(_bits(want), _bits(ref.wetted(sc1.surface, sc1.collision, sc1.dx, cos)))
        kap = s.array("surfaceCurvature").reshape(sc.surface.shape)
        kref = ref.curvature(got, sc.dx)
        assert np.abs(kap - kref).max() <= 1e-5 / sc.dx, np.abs(kap - kref).max() * sc.dx
    finally:
        s.close()


# ---- 4. the force follows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", ["scalar_sigma", "sigma_field"])
def test_rhs_and_b_follow_the_curvature(gpu, switch):
    sc, p = scenes.blob(seed=1)
    sigma = 50.0
    sfield = None
    if switch == "sigma_field":                                     # a sigma field as the only thing that switches the curvature on
        sfield = (sigma * (1.0 + 0.5 * np.random.RandomState(3).uniform(0, 1, sc.surface.shape))).astype(np.float32)
        sc.surface_sigma_field, sc.surface_tension = sfield, 0.0
    else:
        sc.surface_tension = sigma
    try:
        assert gpu.set_contact_angle(-1.0) == abi.SUCCESS
        _run(gpu, sc, p)
        off = gpu.array("activeRHSVector"), gpu.array("reducedRHSVector"), gpu.array("b")
        k_off = gpu.array("surfaceCurvature")
        assert gpu.set_contact_angle(40.0) == abi.SUCCESS
        _run(gpu, sc, p)
        on = gpu.array("activeRHSVector"), gpu.array("reducedRHSVector"), gpu.array("b")
        k_on = gpu.array("surfaceCurvature")
        assert (k_on != k_off).any()
        flat = None if sfield is None else sfield.ravel()
        q_on, q_off = (sref.ghost_pressure(k, sigma_field=flat, sigma=sigma) for k in (k_on, k_off))
        a1, r1, _, b1 = sref.expected_changes(gpu, sc, q_on)
        a0, r0, _, b0 = sref.expected_changes(gpu, sc, q_off)       # (same weights and labels: only the curvature differs)
        assert np.abs(a1 - a0).max() > 0 and np.abs(b1 - b0).max() > 0
        for got, want, big in ((on[0] - off[0], a1 - a0, np.abs(on[0]).max()), (on[1] - off[1], (r1 - r0).ravel(), np.abs(on[1]).max()),
                               (on[2] - off[2], b1 - b0, np.abs(on[2]).max())):
            assert np.abs(got - want).max() <= 1e-12 * max(big, np.abs(want).max()), np.abs(got - want).max()
    finally:
        gpu.set_contact_angle(-1.0)
        gpu.set_surface_tension(0.0)


# ---- 5. direction ------------------------------------------------------------------------------------------------------------------------
# The liquid's viscosity is the one thing the scene leaves open.  The measure sits on the two cell layers above a no-slip floor, so it needs a
# liquid whose momentum diffuses less than a cell per step: mu = 1 with rho = 1000, dt = 1/24, dx = 1/32 gives nu dt / dx^2 = 0.043.  With
# the droplet scenes' mu = 50 (nu dt / dx^2 = 2.1) the floor holds both layers and the third ordering below does NOT hold: measured on an
# MI355X (low side, high side; profiles/contact_angle.md): off -4.1e-5 / +4.1e-5, 60 deg -9.5e-5 / +9.5e-5, 90 deg +2.0e-4 / -2.0e-4,
# 120 deg +8.9e-4 / -8.9e-4: the signs at 60 and 120 degrees are right, but the rule's own inward pull at 90 degrees (its solid cells
# see the kink of the rewritten SDF) exceeds the outward flow at 60.  With mu = 1: off -7.1e-5, 60 deg -8.8e-4, 90 deg +5.9e-4, 120 deg
# +3.0e-3 on the low side, mirrored on the high side.
FOOT_VISCOSITY = 1.0


def foot_flow(solver, deg, viscosity=FOOT_VISCOSITY):
    """(mean u_x on the low-x side, on the high-x side) over the x faces inside the liquid within 3 cells of the contact line, on the two
    cell layers above the floor, in the two cell layers around the centre plane z = 0.5.  The contact line crosses that plane at
    x = 0.5 -+ 0.3, i.e. at the face positions 6.4 and 25.6: the faces inside the liquid are i = 7, 8, 9 and i = 23, 24, 25."""
    sc, p = scenes.sessile_drop(ref.HEMI_N, ref.HEMI_R, ref.HEMI_FLOOR, sigma=1.0, contact_angle=deg, viscosity=viscosity)
    p.tolerance, p.maxSolverIterations = 1e-8, 50000
    _run(solver, sc, p)
    vx = solver.vel[0]
    c = [ref.HEMI_N // 2 - 1, ref.HEMI_N // 2]
    layers = slice(ref.HEMI_FLOOR, ref.HEMI_FLOOR + 2)
    lo = float(vx[c][:, layers, 7:10].astype(np.float64).mean())
    hi = float(vx[c][:, layers, 23:26].astype(np.float64).mean())
    return lo, hi


def test_foot_spreads_below_90_and_retracts_above(gpu):
    try:
        flow = {deg: foot_flow(gpu, deg) for deg in (60.0, 90.0, 120.0)}
    finally:
        gpu.set_contact_angle(-1.0)
        gpu.set_surface_tension(0.0)
    print("foot flow (low side, high side):", flow)
    lo60, hi60 = flow[60.0]
    lo120, hi120 = flow[120.0]
    assert lo60 < 0 < hi60, flow                                    # outward on both sides: it spreads
    assert hi120 < 0 < lo120, flow                                  # inward on both sides: it retracts
    for side in (0, 1):
        assert abs(flow[90.0][side]) < min(abs(flow[60.0][side]), abs(flow[120.0][side])), flow


# ---- 6. memory ---------------------------------------------------------------------------------------------------------------------------
def test_memory_is_flat_and_released_with_the_setting():
    sc, p = scenes.blob(seed=2)
    sc.surface_tension = 1.0
    nc = sc.nx * sc.ny * sc.nz
    s = polystokes_amd.Solver(0)
    try:
        s.upload(sc, p)
        s.step_device()
        s.step_device()
        base = s.memory_stats()["live_bytes"]
        assert s.set_contact_angle(60.0) == abi.SUCCESS
        assert s.memory_stats()["live_bytes"] == base              # the setting alone allocates nothing
        seen = []
        for _ in range(3):
            assert s.step_device() == abi.SUCCESS
            mem = s.memory_stats()
            assert mem["deferred_bytes"] == 0
            seen.append(mem["live_bytes"])
        assert len(set(seen)) == 1, seen
        blocks = -(-sc.nx // 16) * -(-sc.ny // 4) * -(-sc.nz // 4)
        assert seen[0] - base == 2 * 4 * nc + blocks + 4, seen[0] - base        # include/polystokes.h: two fp32 cell grids, flags, a counter
        dev = _hip.DeviceBuffer.from_numpy(np.zeros(nc, np.float32))
        assert s.upload_contact_cosine_field_device(dev) == abi.SUCCESS
        mem = s.memory_stats()
        assert mem["deferred_bytes"] == 0 and mem["live_bytes"] == seen[0] + 4 * nc      # one fp32 cell grid while present
        assert s.set_contact_angle(-1.0) == abi.SUCCESS                                 # the field still asks for the rule
        assert s.memory_stats()["live_bytes"] == seen[0] + 4 * nc
        assert s.step_device() == abi.SUCCESS and int(s.array("contactField")[0]) == 1
        assert s.set_contact_angle(60.0) == abi.SUCCESS
        assert s.upload_contact_cosine_field(None) == abi.SUCCESS
        dev.close()
        mem = s.memory_stats()
        assert mem["deferred_bytes"] == 0 and mem["live_bytes"] == seen[0]
        assert s.set_contact_angle(-1.0) == abi.SUCCESS                                 # off with no field present: released at once
        mem = s.memory_stats()
        assert mem["deferred_bytes"] == 0 and mem["live_bytes"] == base
        with pytest.raises(KeyError):
            s.array("surfaceWetted")
        assert s.step_device() == abi.SUCCESS
        mem = s.memory_stats()
        assert mem["deferred_bytes"] == 0 and mem["live_bytes"] == base
    finally:
        s.close()


# ---- 7. decompositions -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cut_single():
    sc, p = ref.cut_scene(64)
    sc.vel[1][:] = -0.2
    sc.surface_tension, sc.contact_angle = 1.0, 60.0
    s = polystokes_amd.Solver(0)
    try:
        _run(s, sc, p)
        assert float(s.array("contactAngle")[0]) == 60.0
        out = dict(kap=s.array("surfaceCurvature").reshape(sc.surface.shape), vel=[v.copy() for v in s.vel], valid=[v.copy() for v in s.valid])
        U = ref.update_set(sc.collision, sc.dx)
        assert int(s.array("contactCells")[0]) == int(U.sum())
        assert U[30:34, 5:, :].any()                                # the solid sphere crosses the cut above the floor
    finally:
        s.close()
    return sc, p, out


@pytest.mark.parametrize("dims", [None, (2, 2, 2)])
def test_decompositions_match_single_domain(cut_single, dims):
    from test_gpu_surface_tension import _owned_boxes
    sc, p, single = cut_single
    world = 2 if dims is None else 8
    grp = polystokes_amd.Group(world, dims=dims)
    try:
        rc = grp.solve_scene(sc, p)
        assert rc == abi.SUCCESS
        for r, (loc, glob) in zip(grp.ranks, _owned_boxes(world, dims, sc, p)):
            assert float(r.array("contactAngle")[0]) == 60.0 and int(r.array("contactCells")[0]) > 0
            sh = abi.grid_shapes(r.scene.nx, r.scene.ny, r.scene.nz)["center"]
            assert np.array_equal(_bits(r.array("surfaceCurvature").reshape(sh)[loc]), _bits(single["kap"][glob]))
        for a in range(3):
            assert np.array_equal(grp.valid[a], single["valid"][a])
            scale = max(np.abs(single["vel"][a]).max(), 1e-30)
            assert np.abs(grp.vel[a] - single["vel"][a]).max() <= 20 * p.tolerance * scale
    finally:
        grp.close()

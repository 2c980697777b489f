"""Free-surface fields (ps_upload_surface_fields) on the GPU: a surface-tension coefficient and an ambient pressure per cell.

The oracle knows no surface term, so every check is the numpy restatement of tests/surface_fields_ref.py, a byte comparison with a
context that never saw a field, or a closed form: a uniform ambient pressure changes the pressure and nothing else, a pressure gradient
accelerates the droplet rigidly."""
import ctypes as C

import numpy as np
import pytest

import polystokes_amd
from polystokes_amd import _abi as abi
from polystokes_amd import scenes
import surface_fields_ref as ref

pytestmark = pytest.mark.gpu

RHS_NAMES = ("activeRHSVector", "reducedRHSVector", "b")


@pytest.fixture(scope="module")
def gpu():
    s = polystokes_amd.Solver(0)
    yield s
    s.close()


def _cells(sc):
    return (sc.nz, sc.ny, sc.nx)


def _seeded_fields(sc, seed=11):
    """(sigma in [0, 2], pressure in [-500, 500]) per cell"""
    rng = np.random.RandomState(seed)
    return (rng.uniform(0.0, 2.0, _cells(sc)).astype(np.float32), rng.uniform(-500.0, 500.0, _cells(sc)).astype(np.float32))


def _upload(s, sc, p, sigma_field=None, pressure_field=None, sigma=0.0):
    assert s.set_surface_tension(sigma) == abi.SUCCESS
    s.upload(sc, p)
    if sigma_field is not None or pressure_field is not None:
        assert s.upload_surface_fields(sigma_field, pressure_field) == abi.SUCCESS, s.last_error()


def _setup(s, sc, p, **kw):
    _upload(s, sc, p, **kw)
    assert s.setup() == abi.SUCCESS
    return [s.array(n) for n in RHS_NAMES]


def _step(s, sc, p, **kw):
    _upload(s, sc, p, **kw)
    rc = s.step_device()
    assert rc == abi.SUCCESS, (rc, s.last_error())
    s.download()


def _close(got, want, scale):
    assert np.abs(got - want).max(initial=0.0) <= 1e-12 * scale, (np.abs(got - want).max(), scale)


# ---- 1. API and lifetime --------------------------------------------------------------------------------------------------
def test_api_and_lifetime():
    s = polystokes_amd.Solver(0)
    try:
        sc, p = scenes.droplet(24)
        sig, pres = _seeded_fields(sc)
        sf = abi.SurfaceFields(sig.ctypes.data, pres.ctypes.data)
        assert s.L.ps_upload_surface_fields(s.h, C.byref(sf)) == abi.INVALID                    # before any upload
        assert s.last_error() == "ps_upload_surface_fields: call ps_upload_fields first"
        assert s.L.ps_upload_surface_fields_device(s.h, C.byref(sf), 0, None) == abi.INVALID
        s.upload(sc, p)

        def fields_used():
            assert s.setup() == abi.SUCCESS
            return int(s.array("surfaceFields")[0])

        assert fields_used() == 0
        lo, hi = 7 + sc.nx * (3 + sc.ny * 5), 2 + sc.nx * (1 + sc.ny * 9)                      # two cells, lo < hi in x-fastest numbering
        for bad in (np.nan, np.inf, -np.inf, -1.0, -1e-30):
            assert s.upload_surface_fields(sig, pres) == abi.SUCCESS
            b = sig.copy()
            b[9, 1, 2] = b[5, 3, 7] = bad
            assert s.upload_surface_fields(b, pres) == abi.INVALID, bad
            assert s.last_error() == "ps_upload_surface_fields: sigma: non-finite or negative value at cell %d" % lo, s.last_error()
            assert fields_used() == 0                                                           # both fields are dropped
            with pytest.raises(KeyError):
                s.array("surfaceGhostPressure")
        for bad in (np.nan, -np.inf):
            assert s.upload_surface_fields(sig, pres) == abi.SUCCESS
            b = pres.copy()
            b[9, 1, 2] = b[5, 3, 7] = bad
            assert s.upload_surface_fields(sig, b) == abi.INVALID, bad
            assert s.last_error() == "ps_upload_surface_fields: pressure: non-finite value at cell %d" % lo
            assert fields_used() == 0
            assert s.upload_surface_fields(None, b) == abi.INVALID                              # ... also as the only member
            assert fields_used() == 0
        b, c = sig.copy(), pres.copy()                                                          # sigma is checked first
        b.flat[hi], c.flat[lo] = -2.0, np.nan
        assert s.upload_surface_fields(b, c) == abi.INVALID
        assert s.last_error().endswith("sigma: non-finite or negative value at cell %d" % hi)
        b = sig.copy()
        b.flat[lo] = -0.0                                                                       # -0 is not negative; a negative pressure is legal
        assert s.upload_surface_fields(b, -np.abs(pres)) == abi.SUCCESS, s.last_error()

        # a NULL member means absent, not "keep"; surfaceFields reads what the last setup used
        n = sc.nx * sc.ny * sc.nz
        assert s.upload_surface_fields(sig, pres) == abi.SUCCESS and fields_used() == 3
        assert s.array("surfaceGhostPressure").size == n and s.array("surfaceCurvature").size == n
        assert s.upload_surface_fields(sig, None) == abi.SUCCESS and fields_used() == 1
        assert s.array("surfaceGhostPressure").dtype == np.float64 and s.array("surfaceCurvature").size == n
        assert s.upload_surface_fields(None, pres) == abi.SUCCESS and fields_used() == 2
        assert s.array("surfaceTensionReducedFaces").size == 1 and float(s.array("surfaceTension")[0]) == 0.0
        with pytest.raises(KeyError):
            s.array("surfaceCurvature")                                                         # scalar 0 and no sigma field: no curvature
        assert fields_used() == 2                                                               # a second setup without an upload keeps them
        assert s.upload_surface_fields(None, None) == abi.SUCCESS and fields_used() == 0
        assert s.upload_surface_fields(sig, pres) == abi.SUCCESS
        assert s.L.ps_upload_surface_fields(s.h, None) == abi.SUCCESS and fields_used() == 0    # f == NULL drops them
        for name in ("surfaceGhostPressure", "surfaceCurvature", "surfaceTensionReducedFaces"):
            with pytest.raises(KeyError):
                s.array(name)
        # a field upload drops the fields
        assert s.upload_surface_fields(sig, pres) == abi.SUCCESS and fields_used() == 3
        s.upload(sc, p)
        assert fields_used() == 0
        # a scene's fields go with Solver.upload
        sc.surface_sigma_field, sc.surface_pressure_field = sig, None
        s.upload(sc, p)
        assert fields_used() == 1
    finally:
        s.close()


# ---- 2. right-hand sides against numpy ------------------------------------------------------------------------------------
def _rhs_scene(name):
    if name == "blob":
        return scenes.blob(seed=0)
    if name == "droplet":
        return scenes.droplet(24)
    sc, p = scenes.droplet(32)                              # tests/test_gpu_surface_tension.py: test_reduced_faces_next_to_the_surface
    p.activeLiquidBoundaryLayerSize, p.tilePadding = 0, 1
    return sc, p


@pytest.fixture(scope="module")
def rhs_base(gpu):
    """per scene: (scene, params, the three rhs vectors of a setup without any surface term), computed once"""
    out = {}
    for name in ("blob", "droplet", "tiles_at_the_surface"):
        sc, p = _rhs_scene(name)
        out[name] = (sc, p, _setup(gpu, sc, p))
    return out


@pytest.mark.parametrize("which", ["sigma", "pressure", "both"])
@pytest.mark.parametrize("name", ["blob", "droplet", "tiles_at_the_surface"])
def test_rhs_against_numpy(gpu, rhs_base, name, which):
    sc, p, (rhs0, rr0, b0) = rhs_base[name]
    sig, pres = _seeded_fields(sc)
    sig, pres = (sig if which != "pressure" else None), (pres if which != "sigma" else None)
    rhs1, rr1, b1 = _setup(gpu, sc, p, sigma_field=sig, pressure_field=pres)
    assert int(gpu.array("surfaceFields")[0]) == {"sigma": 1, "pressure": 2, "both": 3}[which]
    kap = gpu.array("surfaceCurvature").reshape(_cells(sc)) if sig is not None else None
    q_want = ref.ghost_pressure(kap, sig, 0.0, pres)
    q = gpu.array("surfaceGhostPressure")
    assert q.tobytes() == q_want.tobytes()                                                       # bit for bit
    d_a, d_r, hits, d_b = ref.expected_changes(gpu, sc, q)
    assert np.abs(d_a).max() > 1.0
    _close(rhs1 - rhs0, d_a, max(np.abs(rhs1).max(), np.abs(d_a).max()))
    assert int(gpu.array("surfaceTensionReducedFaces")[0]) == hits
    if name == "tiles_at_the_surface":
        assert hits > 0 and np.abs(d_r).max() > 0                                                # reduced faces carry impulses
    _close(rr1 - rr0, d_r.ravel(), max(np.abs(rr1).max(), np.abs(d_r).max(), 1e-300))
    _close(b1 - b0, d_b, max(np.abs(b1).max(), np.abs(d_b).max()))


# ---- 3. absent means untouched --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.0, 2.0])
def test_dropped_fields_leave_the_step_untouched(sigma):
    sc, p = scenes.droplet(32)
    sc.vel[1][:] = -0.3                                             # something to project
    sig, pres = _seeded_fields(sc)
    a, b = polystokes_amd.Solver(0), polystokes_amd.Solver(0)
    try:
        _step(a, sc, p, sigma=sigma)
        _step(b, sc, p, sigma_field=sig, pressure_field=pres, sigma=sigma)      # a step with both fields first
        assert int(b.array("surfaceFields")[0]) == 3 and not np.array_equal(a.array("b"), b.array("b"))
        _upload(b, sc, p, sigma_field=sig, pressure_field=pres, sigma=sigma)
        assert b.upload_surface_fields(None, None) == abi.SUCCESS               # uploaded, then dropped
        assert b.step_device() == abi.SUCCESS
        b.download()
        assert int(b.array("surfaceFields")[0]) == 0
        for name in ("activeRHSVector", "reducedRHSVector", "b", "solutionVector"):
            assert a.array(name).tobytes() == b.array(name).tobytes(), name
        for q in range(3):
            assert a.vel[q].tobytes() == b.vel[q].tobytes()
    finally:
        a.close()
        b.close()


# ---- 4. a constant sigma field is the scalar ------------------------------------------------------------------------------
@pytest.mark.parametrize("v", [0.07, 2.0])
def test_constant_sigma_field_against_the_scalar(gpu, v):
    sc, p = scenes.blob(seed=0)
    try:
        want = _setup(gpu, sc, p, sigma=v)
        assert int(gpu.array("surfaceFields")[0]) == 0
        got = _setup(gpu, sc, p, sigma_field=np.full(_cells(sc), v, np.float32))
        assert int(gpu.array("surfaceFields")[0]) == 1
        # the field holds fp32(v), the scalar v: 0.07 differs from its fp32 rounding by 2.4e-9 relative, so the scalar run uses fp32(v) too
        if float(np.float32(v)) != v:
            want = _setup(gpu, sc, p, sigma=float(np.float32(v)))
        for g, w in zip(got, want):
            _close(g, w, np.abs(w).max())
    finally:
        gpu.set_surface_tension(0.0)


# ---- 5. a uniform ambient pressure changes nothing but the pressure -------------------------------------------------------
# The bounds of tests/test_gpu_surface_tension.py (LAPLACE_P_TOL, LAPLACE_U_TOL, LAPLACE_TILES_P_TOL, LAPLACE_TILES_U_TOL), copied: its
# Laplace tests are this experiment with a ghost pressure that additionally carries the curvature's noise.
LAPLACE_P_TOL = 0.001
LAPLACE_U_TOL = 0.06
LAPLACE_TILES_P_TOL = 0.001
LAPLACE_TILES_U_TOL = 0.04


def _uniform_pressure(P=1000.0, n=48, liquid_layers=None, pad=2):
    """(|mean interior pressure / P - 1|, max|u| / (dt P / (rho dx))) of the resting droplet under the ambient pressure P, measured as
    laplace() of tests/test_gpu_surface_tension.py measures them, on the same interior mask"""
    sc, p = scenes.droplet(n, pad=pad)
    p.tolerance, p.maxSolverIterations = 1e-8, 50000
    if liquid_layers is not None:
        p.activeLiquidBoundaryLayerSize = liquid_layers
    s = polystokes_amd.Solver(0)
    try:
        _step(s, sc, p, pressure_field=np.full(_cells(sc), P, np.float32))
        assert int(s.array("surfaceFields")[0]) == 2
        pr = s.solution_fields()["pressure"]
        lab = s.array("centerLabels").reshape(pr.shape)
        inner = (sc.surface < -3 * sc.dx) & ref.active_label(lab)
        assert inner.sum() > 100
        pe = abs(pr[inner].astype(np.float64).mean() / P - 1)
        U = sc.dt * P / (sc.density * sc.dx)
        umax = max(np.abs(v).max() for v in s.vel)
        return pe, umax / U
    finally:
        s.close()


def test_uniform_ambient_pressure_changes_only_the_pressure():
    pe, ur = _uniform_pressure()
    print("uniform ambient pressure: pe = %.3e, ur = %.3e" % (pe, ur))
    assert pe <= LAPLACE_P_TOL, pe
    assert ur <= LAPLACE_U_TOL, ur


def test_uniform_ambient_pressure_with_tiles_at_the_surface():
    pe, ur = _uniform_pressure(liquid_layers=0, pad=1)
    print("uniform ambient pressure, tiles at the surface: pe = %.3e, ur = %.3e" % (pe, ur))
    assert pe <= LAPLACE_TILES_P_TOL, pe
    assert ur <= LAPLACE_TILES_U_TOL, ur


# ---- 6. direction ---------------------------------------------------------------------------------------------------------
def _mean_vx_inside(s, sc):
    """mean of vx over the x faces between two cells whose SDF, averaged to the face, lies below -2 dx"""
    phi = 0.5 * (sc.surface[:, :, 1:] + sc.surface[:, :, :-1])
    inside = phi < -2 * sc.dx
    assert inside.sum() > 1000
    return float(s.vel[0][:, :, 1:-1][inside].astype(np.float64).mean())


def test_liquid_moves_toward_the_lower_sigma(gpu):
    """sigma 2 on the half x > 0.5, 1 on the other: the higher curvature pressure on the right pushes the droplet toward -x"""
    sc, p = scenes.droplet(32)
    p.tolerance = 1e-8
    x = (np.arange(sc.nx) + 0.5) * sc.dx
    sig = np.broadcast_to(np.where(x > 0.5, 2.0, 1.0).astype(np.float32), _cells(sc))
    _step(gpu, sc, p, sigma_field=sig)
    assert _mean_vx_inside(gpu, sc) < 0


def test_pressure_gradient_accelerates_the_droplet_rigidly(gpu):
    """P = a x at the cell centres, sigma 0: the continuum problem is a rigid acceleration -a / rho, so the mean vx after one step is
    -dt a / rho.  Measured ratio: profiles/surface_fields.md."""
    sc, p = scenes.droplet(32)
    p.tolerance = 1e-8
    a = 1000.0
    x = (np.arange(sc.nx) + 0.5) * sc.dx
    _step(gpu, sc, p, pressure_field=np.broadcast_to((a * x).astype(np.float32), _cells(sc)))
    mean = _mean_vx_inside(gpu, sc)
    ratio = mean / (-sc.dt * a / sc.density)
    print("pressure gradient: mean vx / (-dt a / rho) = %.4f" % ratio)
    assert mean < 0
    assert 0.5 <= ratio <= 2.0, ratio


# ---- 7. device-resident upload --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [abi.LAYOUT_X_FASTEST, abi.LAYOUT_Z_FASTEST])
def test_device_upload_equals_the_host_upload(gpu, layout):
    sc, p = scenes.blob(seed=0)
    sig, pres = _seeded_fields(sc)
    want = _setup(gpu, sc, p, sigma_field=sig, pressure_field=pres)
    q_want = gpu.array("surfaceGhostPressure")
    sc.surface_sigma_field, sc.surface_pressure_field = sig, pres
    ds = polystokes_amd.device_scene(sc, layout)
    s = polystokes_amd.Solver(0)
    try:
        assert s.upload_device(p, ds, layout) == abi.SUCCESS, s.last_error()
        assert s.upload_surface_fields_device(ds.surface_sigma_field, ds.surface_pressure_field, layout) == abi.SUCCESS, s.last_error()
        assert s.setup() == abi.SUCCESS
        assert int(s.array("surfaceFields")[0]) == 3
        assert s.array("surfaceGhostPressure").tobytes() == q_want.tobytes()
        for name, w in zip(RHS_NAMES, want):
            assert s.array(name).tobytes() == w.tobytes(), name
        # one member alone
        assert s.upload_surface_fields_device(None, ds.surface_pressure_field, layout) == abi.SUCCESS
        assert s.setup() == abi.SUCCESS and int(s.array("surfaceFields")[0]) == 2
    finally:
        s.close()


def test_device_upload_refusals_and_the_index_of_a_bad_value():
    from polystokes_amd import _hip
    sc, p = scenes.blob(seed=0)
    sig, pres = _seeded_fields(sc)
    bad_s, bad_p = sig.copy(), pres.copy()
    bad_s[5, 3, 7] = -1.0
    bad_s[9, 1, 2] = np.nan                          # a later one in x-fastest order, an earlier one in z-fastest order
    bad_p[5, 3, 7] = bad_p[9, 1, 2] = np.inf
    cell = 7 + sc.nx * (3 + sc.ny * 5)
    s = polystokes_amd.Solver(0)
    try:
        for layout in (abi.LAYOUT_X_FASTEST, abi.LAYOUT_Z_FASTEST):
            ds = polystokes_amd.device_scene(sc, layout)
            assert s.upload_device(p, ds, layout) == abi.SUCCESS
            put = lambda a, pad=0: _hip.DeviceBuffer.from_numpy(polystokes_amd.to_layout(a, layout), pad)
            good_s, good_p = put(sig), put(pres, 1)                               # (a pointer that is only 4-byte aligned is fine)
            assert s.upload_surface_fields_device(good_s, good_p, layout) == abi.SUCCESS, s.last_error()
            assert s.upload_surface_fields_device(put(bad_s), good_p, layout) == abi.INVALID
            assert s.last_error() == "ps_upload_surface_fields: sigma: non-finite or negative value at cell %d" % cell
            assert s.upload_surface_fields_device(good_s, put(bad_p), layout) == abi.INVALID
            assert s.last_error() == "ps_upload_surface_fields: pressure: non-finite value at cell %d" % cell
            assert s.setup() == abi.SUCCESS and int(s.array("surfaceFields")[0]) == 0
            # the refusals of ps_upload_density_field_device, decided before anything is read through a pointer; each drops both fields
            assert s.upload_surface_fields_device(good_s, good_p, layout) == abi.SUCCESS
            assert s.upload_surface_fields_device(good_s, good_p, 2) == abi.INVALID
            assert s.last_error() == "ps_upload_surface_fields_device: layout must be 0 (x fastest) or 1 (z fastest)"
            assert s.upload_surface_fields_device(good_s, good_p, layout) == abi.SUCCESS
            assert s.upload_surface_fields_device(good_s.ptr + 2, good_p, layout) == abi.INVALID
            assert s.last_error() == "ps_upload_surface_fields_device: sigma: the pointer is not 4-byte aligned"
            assert s.upload_surface_fields_device(good_s, good_p, layout) == abi.SUCCESS
            assert s.upload_surface_fields_device(good_s, sig.ctypes.data, layout) == abi.INVALID
            assert s.last_error() == "ps_upload_surface_fields_device: pressure: the pointer is not device memory of the context's device"
            assert s.upload_surface_fields_device(good_s, good_p, layout) == abi.SUCCESS
            assert s.upload_surface_fields_device(good_s.ptr + 4, good_p, layout) == abi.INVALID
            assert "sigma: the allocation ends before the field does" in s.last_error()
            assert s.setup() == abi.SUCCESS and int(s.array("surfaceFields")[0]) == 0
    finally:
        s.close()


# ---- 8. decompositions ----------------------------------------------------------------------------------------------------
def _owned_boxes(world, dims, sc, p):
    """per rank: (local slices of the owned cells, global slices of the same cells)"""
    from polystokes_amd import partition
    out = []
    for r in range(world):
        if dims is None:
            sl = partition.make_slab(sc.nz, world, r, p.tileSize)
            out.append(((slice(sl.zLoOwned, sl.zHiOwned), slice(None), slice(None)),
                        (slice(sl.g0 + sl.zLoOwned, sl.g0 + sl.zHiOwned), slice(None), slice(None))))
        else:
            b = partition.make_brick((sc.nx, sc.ny, sc.nz), dims, r, p.tileSize)
            out.append((tuple(slice(b.lo[a], b.hi[a]) for a in (2, 1, 0)),
                        tuple(slice(b.origin[a] + b.lo[a], b.origin[a] + b.hi[a]) for a in (2, 1, 0))))
    return out


@pytest.mark.parametrize("dims", [None, (2, 2, 2)])
def test_decompositions_match_single_domain(dims):
    world = 2 if dims is None else 8
    sc, p = scenes.droplet(32, tile=8)
    sc.vel[1][:] = -0.2                                             # something to project
    sc.surface_sigma_field, sc.surface_pressure_field = _seeded_fields(sc)
    single = polystokes_amd.Solver(0)
    grp = polystokes_amd.Group(world, dims=dims)
    try:
        assert single.step(sc, p) == abi.SUCCESS
        assert int(single.array("surfaceFields")[0]) == 3
        q = single.array("surfaceGhostPressure").reshape(_cells(sc))
        assert grp.solve_scene(sc, p) == abi.SUCCESS
        for r, (loc, glob) in zip(grp.ranks, _owned_boxes(world, dims, sc, p)):
            assert int(r.array("surfaceFields")[0]) == 3
            sh = abi.grid_shapes(r.scene.nx, r.scene.ny, r.scene.nz)["center"]
            assert r.array("surfaceGhostPressure").reshape(sh)[loc].tobytes() == np.ascontiguousarray(q[glob]).tobytes()
        for a in range(3):
            assert np.array_equal(grp.valid[a], single.valid[a])
            scale = max(np.abs(single.vel[a]).max(), 1e-30)
            assert np.abs(grp.vel[a] - single.vel[a]).max() <= 20 * p.tolerance * scale
    finally:
        grp.close()
        single.close()


# ---- 9. memory ------------------------------------------------------------------------------------------------------------
def test_memory_of_the_fields():
    sc, p = scenes.droplet(24)
    n = sc.nx * sc.ny * sc.nz
    sig, pres = _seeded_fields(sc)
    s = polystokes_amd.Solver(0)

    def live():
        m = s.memory_stats()
        assert m["deferred_bytes"] == 0
        return m["live_bytes"]
    try:
        s.set_surface_tension(1.0)                                  # the curvature buffers are the scalar's: they belong to the base
        s.upload(sc, p)
        assert s.setup() == abi.SUCCESS
        base = live()
        assert s.upload_surface_fields(sig, pres) == abi.SUCCESS
        assert live() == base + 4 * n + 4 * n                       # the two fp32 grids; q comes with the setup
        assert s.setup() == abi.SUCCESS
        assert live() == base + 4 * n + 4 * n + 8 * n
        assert s.setup() == abi.SUCCESS and live() == base + 16 * n
        assert s.upload_surface_fields(None, None) == abi.SUCCESS
        assert live() == base
        assert s.upload_surface_fields(None, pres) == abi.SUCCESS and s.setup() == abi.SUCCESS
        assert live() == base + 4 * n + 8 * n
        bad = sig.copy()
        bad.flat[17] = np.nan
        assert s.upload_surface_fields(bad, pres) == abi.INVALID    # a refusal releases them too
        assert live() == base
        assert s.upload_surface_fields(sig, pres) == abi.SUCCESS and s.setup() == abi.SUCCESS
        s.upload(sc, p)                                             # ... and so does a field upload
        assert live() == base
        assert s.setup() == abi.SUCCESS and live() == base
    finally:
        s.close()

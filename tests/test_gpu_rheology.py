"""Non-Newtonian viscosity (ps_set_rheology) on the GPU.

The strain rate and the viscosity are checked against the numpy restatement (rheology_ref.py) computed from the uploaded velocity and the
step's `valid` flags; the solve is checked against the uploaded-field path, which the oracle covers elsewhere: a second context given the
computed viscosity as its field solves the same system."""
import os

import numpy as np
import pytest

from polystokes_amd import _abi as abi
from polystokes_amd import scenes

import children
import rheology_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HB, NEWTON = abi.RHEOLOGY_HERSCHEL_BULKLEY, abi.RHEOLOGY_NEWTONIAN
LAW = dict(min_shear_rate=1e-2, min_viscosity=1e-3, max_viscosity=1e5)


def _solver(**rh):
    import polystokes_amd
    s = polystokes_amd.Solver(0)
    if rh:
        assert s.set_rheology(**rh) == abi.SUCCESS, s.last_error()
    return s


def _run(s, sc, p, want=abi.SUCCESS):
    rc = s.step(sc, p)
    assert rc == want, (rc, s.last_error())
    return rc


def _swirl(sc, amp=0.5):
    """a smooth velocity on top of the scene's, so that the bulk has a strain rate (coil and cavity are uniform / a lid row)"""
    for a in range(3):
        zz, yy, xx = np.meshgrid(*[np.arange(m) * sc.dx for m in sc.vel[a].shape], indexing="ij")
        sc.vel[a] += (amp * np.sin(6 * xx + a) * np.cos(5 * yy - a) * np.sin(4 * zz + 0.5 * a)).astype(np.float32)
    return sc


def _scene(name):
    if name == "blob":
        return scenes.blob()                                   # variable K
    if name == "coil":
        sc, p = scenes.coil(32, tile=8)
        return _swirl(sc), p
    if name == "cavity":
        sc, p = scenes.cavity(64)
        return _swirl(sc), p
    return scenes.spheres(32, tile=8)


def _relvel(a, b):
    return max(np.abs(a[q] - b[q]).max() / max(np.abs(b[q]).max(), 1e-30) for q in range(3))


def _numpy_fields(s, sc, vel, n, tau, law=LAW):
    return ref.fields(vel, s.valid, sc.dx, sc.viscosity, n, tau, law["min_shear_rate"], law["min_viscosity"], law["max_viscosity"])


def _with_viscosity(sc, mu):
    sc2 = abi.Scene(sc.nx, sc.ny, sc.nz, sc.dx, sc.dt, sc.density, sc.vel, sc.surface, sc.collision, mu, collisionvel=sc.collisionvel,
                    name=sc.name + "_mu", density_field=sc.density_field, surface_tension=sc.surface_tension)
    return sc2


# ---- 1. the setting ----------------------------------------------------------------------------------------------------------
def test_bad_values_keep_the_setting_and_it_persists():
    sc, p = scenes.blob()
    s = _solver()
    try:
        s.upload(sc, p)
        assert s.setup() == abi.SUCCESS
        assert int(s.array("rheologyModel")[0]) == NEWTON                 # the default
        with pytest.raises(KeyError):
            s.array("rheologyViscosity")
        assert s.set_rheology(flow_index=0.5, yield_stress=1.0, **LAW) == abi.SUCCESS
        bad = [dict(model=2), dict(model=-1), dict(passes=9), dict(passes=-1), dict(flow_index=0.0), dict(flow_index=4.5),
               dict(flow_index=float("nan")), dict(yield_stress=-1.0), dict(yield_stress=float("inf")), dict(min_shear_rate=0.0),
               dict(min_viscosity=0.0), dict(min_viscosity=2.0, max_viscosity=1.0), dict(max_viscosity=float("inf"))]
        for b in bad:
            kw = dict(flow_index=0.5, **LAW)
            kw.update(b)
            assert s.set_rheology(**kw) == abi.INVALID, b
            assert "ps_set_rheology" in s.last_error(), b
        assert s.L.ps_set_rheology(s.h, None) == abi.INVALID
        s.upload(sc, p)                                                  # the setting persists across uploads
        assert s.setup() == abi.SUCCESS
        assert int(s.array("rheologyModel")[0]) == HB
        rate = s.array("rheologyStrainRate")
        mu = s.array("rheologyViscosity")
        assert rate.size == mu.size == sc.nx * sc.ny * sc.nz
        assert np.all(np.isfinite(mu)) and mu.min() >= 1e-3 and mu.max() <= 1e5      # the kept setting's clamps
        assert s.set_rheology(model=NEWTON) == abi.SUCCESS
        s.upload(sc, p)
        assert s.setup() == abi.SUCCESS
        assert int(s.array("rheologyModel")[0]) == NEWTON
    finally:
        s.close()


@pytest.mark.parametrize("name", ["coil", "spheres"])
def test_newtonian_setting_is_the_default_path(name):
    sc, p = _scene(name)
    a, b = _solver(), _solver(model=NEWTON, flow_index=0.5, yield_stress=3.0, passes=4)    # the other members are ignored
    try:
        _run(a, sc, p)
        _run(b, sc, p)
        for q in range(3):
            assert a.vel[q].tobytes() == b.vel[q].tobytes() and a.valid[q].tobytes() == b.valid[q].tobytes()
        assert a.array("solutionVector").tobytes() == b.array("solutionVector").tobytes()
        assert int(b.array("rheologyModel")[0]) == NEWTON
        for name_ in ("rheologyViscosity", "rheologyStrainRate", "rheologyIterations"):
            with pytest.raises(KeyError):
                b.array(name_)
    finally:
        a.close()
        b.close()


# ---- 2. the fields against numpy --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blob", "coil", "cavity"])
def test_fields_match_numpy(name):
    sc, p = _scene(name)
    s = _solver()
    try:
        for n, tau in ((0.5, 0.0), (1.0, 2.0), (1.6, 0.3), (0.7, 0.0)):
            assert s.set_rheology(flow_index=n, yield_stress=tau, **LAW) == abi.SUCCESS
            _run(s, sc, p)
            rate_np, mu_np = _numpy_fields(s, sc, sc.vel, n, tau)
            rate = s.array("rheologyStrainRate").reshape(rate_np.shape)
            mu = s.array("rheologyViscosity").reshape(mu_np.shape)
            assert rate.max() > 0, (name, n, tau)
            assert ref.ulps(rate, rate_np).max() <= 1, (name, n, tau, ref.ulps(rate, rate_np).max())
            assert ref.ulps(mu, mu_np).max() <= 1, (name, n, tau, ref.ulps(mu, mu_np).max())
            assert list(s.array("rheologyIterations")) == [int(s.stats.solveData[1])]
    finally:
        s.close()


# ---- 3. identity with the uploaded-field path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blob", "coil"])
def test_same_system_as_the_uploaded_field(name):
    """bit for bit: the step is deterministic and both contexts sample the same fp32 field through the same kernels"""
    sc, p = _scene(name)
    a = _solver(flow_index=0.5, yield_stress=0.5, **LAW)
    b = _solver()
    try:
        _run(a, sc, p)
        mu = a.array("rheologyViscosity").reshape(sc.viscosity.shape)
        assert np.unique(mu).size > 256                                  # a genuine field (the fp64 stress diagonal)
        _run(b, _with_viscosity(sc, mu), p)
        assert int(a.stats.solveData[1]) == int(b.stats.solveData[1])
        for q in range(3):
            assert a.vel[q].tobytes() == b.vel[q].tobytes(), q
        assert int(a.array("diagonalsCoded")[0]) == int(b.array("diagonalsCoded")[0])
    finally:
        a.close()
        b.close()


# ---- 4. Newtonian limit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blob", "coil"])
def test_newtonian_limit(name):
    sc, p = _scene(name)
    a = _solver(flow_index=1.0, yield_stress=0.0, min_shear_rate=1e-3, min_viscosity=1e-3, max_viscosity=1e6)
    b = _solver()
    try:
        _run(a, sc, p)
        _run(b, sc, p)
        assert a.array("rheologyViscosity").tobytes() == sc.viscosity.tobytes()
        assert _relvel(a.vel, b.vel) <= 10 * p.tolerance
    finally:
        a.close()
        b.close()


# ---- 5. Picard passes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["coil", "blob"])
def test_one_pass_reads_the_first_solve(name):
    sc, p = _scene(name)
    n, tau = 0.6, 0.2
    a = _solver(flow_index=n, yield_stress=tau, passes=0, **LAW)
    b = _solver(flow_index=n, yield_stress=tau, passes=1, **LAW)
    try:
        _run(a, sc, p)
        _run(b, sc, p)
        _, mu_np = _numpy_fields(a, sc, a.vel, n, tau)                # numpy on the first solve's velocity and valid flags
        mu = b.array("rheologyViscosity").reshape(mu_np.shape)
        assert ref.ulps(mu, mu_np).max() <= 1
        assert np.array_equal(a.valid[0], b.valid[0])
        it = list(b.array("rheologyIterations"))
        assert len(it) == 2 and it[0] == int(a.stats.solveData[1]) and it[1] == int(b.stats.solveData[1])
        assert it[1] < it[0], it                                        # the carried iterate
    finally:
        a.close()
        b.close()


def test_passes_carry_the_iterate_and_sum_the_times():
    sc, p = _scene("coil")
    s = _solver(flow_index=0.7, passes=3, **LAW)
    one = _solver(flow_index=0.7, passes=0, **LAW)
    try:
        _run(one, sc, p)
        _run(s, sc, p)
        it = list(s.array("rheologyIterations"))
        assert len(it) == 4, it
        assert it[0] == int(one.stats.solveData[1])
        assert max(it[1:]) < it[0], it
        assert int(s.stats.solveData[1]) == it[-1]
        assert s.stats.solveData[5] > one.stats.solveData[5]            # setup wall time summed over four setups
        assert sum(s.stats.stage_ms) > sum(one.stats.stage_ms)
        with pytest.raises(KeyError):
            s.array("warmStartVector")                                  # WARM_NONE: the carried iterate served the passes only
    finally:
        s.close()
        one.close()


def test_interrupt_leaves_the_input_velocity():
    sc, p = _scene("coil")
    p.tolerance = 1e-9
    s = _solver(flow_index=0.5, passes=2, **LAW)
    try:
        s.set_interrupt(lambda: True)                                   # the first solve stops
        assert s.step(sc, p) == abi.INCOMPLETE
        for q in range(3):
            assert s.vel[q].tobytes() == sc.vel[q].tobytes()
        # a later pass stops: count the polls of a whole first solve, then stop at the next one
        calls = []
        assert s.set_rheology(flow_index=0.5, passes=0, **LAW) == abi.SUCCESS
        s.set_interrupt(lambda: (calls.append(1), False)[1])
        _run(s, sc, p)
        first = len(calls)
        assert first > 0
        calls.clear()
        assert s.set_rheology(flow_index=0.5, passes=2, **LAW) == abi.SUCCESS
        s.set_interrupt(lambda: (calls.append(1), len(calls) > first)[1])
        assert s.step(sc, p) == abi.INCOMPLETE
        assert len(calls) > first
        for q in range(3):
            assert s.vel[q].tobytes() == sc.vel[q].tobytes()
        s.set_interrupt(None)
    finally:
        s.close()


@pytest.mark.parametrize("name", ["coil", "cavity"])
def test_passes_reduce_the_self_consistency_defect(name):
    sc, p = _scene(name)
    n = 0.7
    defect = {}
    for k in (1, 4):
        s = _solver(flow_index=n, passes=k, **LAW)
        try:
            _run(s, sc, p)
            mu_k = s.array("rheologyViscosity").astype(np.float64)
            _, mu_u = _numpy_fields(s, sc, s.vel, n, 0.0)
            defect[k] = float(np.linalg.norm(mu_u.ravel().astype(np.float64) - mu_k) / np.linalg.norm(mu_k))
        finally:
            s.close()
    print("defect", name, defect)
    assert defect[4] < defect[1], defect


# ---- 6. decompositions --------------------------------------------------------------------------------------------------------
def _owned_cells(grp, sc):
    """(rank, local cell slices, global cell slices) of the owned cells of every rank, numpy (z, y, x) order"""
    out = []
    for r, part in enumerate(grp.slabs):
        if grp.dims is None:
            loc = (slice(part.zLoOwned, part.zHiOwned), slice(None), slice(None))
            glo = (slice(part.z0, part.z1), slice(None), slice(None))
        else:
            loc = tuple(slice(part.lo[a], part.hi[a]) for a in (2, 1, 0))
            glo = tuple(slice(part.g0[a], part.g1[a]) for a in (2, 1, 0))
        out.append((r, loc, glo))
    return out


@pytest.mark.parametrize("dims", [None, (2, 2, 2)])
def test_decompositions_match_single_domain(dims):
    """Every rank computes the single domain's mu on the cells it owns, bit for bit.  The velocities then come from the same system solved
    on another layout: at tolerance 1e-8 the stop rule bounds the residual, not the error, and the law's viscosity contrast (K = 1e4 at
    rest against the sheared liquid) makes the error per residual larger than the Newtonian one.  So they are held to twice what the
    identity preconditioner's solve of the same single-domain system lies from Jacobi's."""
    import polystokes_amd
    world = 2 if dims is None else 8
    sc, p = scenes.spheres(32, tile=8)
    p.tolerance, p.maxSolverIterations = 1e-8, 20000
    law = dict(flow_index=0.7, yield_stress=0.5, **LAW)
    err = {}
    for model in (NEWTON, HB):
        single = _solver(model=model, **law)
        grp = polystokes_amd.Group(world, dims=dims)
        try:
            assert grp.set_rheology(model=model, **law) == abi.SUCCESS
            _run(single, sc, p)
            assert grp.solve_scene(sc, p) == abi.SUCCESS
            for r in grp.ranks:
                assert int(r.array("rheologyModel")[0]) == model
            for a in range(3):
                assert np.array_equal(grp.valid[a], single.valid[a])
            if model == HB:
                mu = single.array("rheologyViscosity").reshape(sc.viscosity.shape)
                for r, loc, glo in _owned_cells(grp, sc):
                    sh = abi.grid_shapes(grp.ranks[r].scene.nx, grp.ranks[r].scene.ny, grp.ranks[r].scene.nz)["center"]
                    mu_r = grp.ranks[r].array("rheologyViscosity").reshape(sh)
                    assert mu_r[loc].tobytes() == mu[glo].tobytes(), r
                    assert list(grp.ranks[r].array("rheologyIterations")) == [int(grp.stats.solveData[1])]
            err[model] = _relvel(grp.vel, single.vel)
        finally:
            grp.close()
            single.close()
    p.preconditioner = abi.PRE_IDENTITY
    ident = _solver(**law)
    jac = _solver(**law)
    try:
        _run(ident, sc, p)
        p.preconditioner = abi.PRE_DIAGONAL
        _run(jac, sc, p)
        spread = _relvel(ident.vel, jac.vel)
    finally:
        ident.close()
        jac.close()
    print("decomposition", dims, err, "identity vs Jacobi", spread)
    assert err[HB] <= max(10 * p.tolerance, 2 * err[NEWTON], 2 * spread), (err, spread)


def test_passes_on_a_group_fail_on_every_rank():
    import polystokes_amd
    sc, p = scenes.spheres(32, tile=8)
    for dims in (None, (2, 2, 2)):
        grp = polystokes_amd.Group(2 if dims is None else 8, dims=dims)
        try:
            assert grp.set_rheology(flow_index=0.7, passes=1, **LAW) == abi.SUCCESS
            with pytest.raises(polystokes_amd.PolyStokesError, match="rheology passes need a single domain"):
                grp.solve_scene(sc, p)
            assert grp.set_rheology(flow_index=0.7, passes=0, **LAW) == abi.SUCCESS      # the first-solve form works
            assert grp.solve_scene(sc, p) == abi.SUCCESS
        finally:
            grp.close()


# ---- 7. robustness ------------------------------------------------------------------------------------------------------------
_CHILD = (
    "import hashlib\n"
    "sc, p = scenes.blob()\n"
    "s = polystokes_amd.Solver(0)\n"
    "s.set_rheology(flow_index=0.6, yield_stress=0.3, passes=2, min_shear_rate=1e-2, min_viscosity=1e-3, max_viscosity=1e5)\n"
    "rc = s.step(sc, p)\n"
    "h = hashlib.sha256(b''.join(v.tobytes() for v in s.vel) + s.array('rheologyViscosity').tobytes()).hexdigest()\n"
    "print('RESULT ' + json.dumps(dict(rc=rc, h=h, it=[int(i) for i in s.array('rheologyIterations')])))\n"
    "s.close()\n"
)


def _child(env):
    return children.run_python(_CHILD, limit=600, env=env).result()


def test_poison_and_release_library_give_the_same_velocities():
    plain = _child({})
    assert plain["rc"] == abi.SUCCESS and len(plain["it"]) == 3
    assert _child({"PS_DEBUG_POISON": "1"}) == plain
    assert _child({"PS_LIB": os.path.join(ROOT, "polystokes_amd", "libpolystokes_hip_release.so")}) == plain


def test_with_surface_tension_free_slip_density_field_and_warm_start():
    sc, p = scenes.sliding_block(32)
    scenes.with_density_field(sc, "layers")
    sc.surface_tension = 0.5
    _swirl(sc, 0.2)
    p.tolerance, p.maxSolverIterations = 1e-7, 20000
    a = _solver(flow_index=0.7, yield_stress=0.5, **LAW)
    b = _solver()
    try:
        for s in (a, b):
            assert s.set_solid_boundary(abi.SOLID_FREE_SLIP) == abi.SUCCESS
            s.set_warm_start(abi.WARM_PREVIOUS_STEP)
        for step in range(2):
            a.upload(sc, p)
            assert a.step_device() == abi.SUCCESS, a.last_error()
            a.download()
            mu = a.array("rheologyViscosity").reshape(sc.viscosity.shape)
            b.upload(_with_viscosity(sc, mu), p)
            assert b.step_device() == abi.SUCCESS, b.last_error()
            b.download()
            assert int(a.array("densityField")[0]) == 1 and float(a.array("surfaceTension")[0]) == 0.5
            assert int(a.array("solidBoundary")[0]) == abi.SOLID_FREE_SLIP
            assert _relvel(a.vel, b.vel) <= 10 * p.tolerance, step
        assert int(a.array("warmStartUsed")[0]) == 1
    finally:
        a.close()
        b.close()

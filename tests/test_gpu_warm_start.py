"""Warm start (ps_set_warm_start) and the solution as grid fields (ps_download_solution_fields) on the GPU.

Mode PS_WARM_PREVIOUS_STEP: a kept single-domain PCG step leaves its [p; tau] on the device as fp32 grids; the next PCG solve on the same grid
starts from them, gathered through the new step's index maps (r0 = b - A x0, pcg.h:284), and runs the unchanged PCG from there."""
import os

import numpy as np
import pytest

from polystokes_amd import _abi as abi
from polystokes_amd import scenes

import children
from helpers import numpy_pcg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECONDS = [abi.PRE_IDENTITY, abi.PRE_DIAGONAL, abi.PRE_CHEBYSHEV, abi.PRE_CHEBYSHEV_F32]


@pytest.fixture(scope="module")
def gpu():
    import polystokes_amd
    s = polystokes_amd.Solver(0)
    yield s
    s.close()


def _new_solver():
    import polystokes_amd
    return polystokes_amd.Solver(0)


def scatter_ref(solver, x):
    """x in reference numbering ([p; txx; tyy; tzz; tyz; txz; txy]) -> the seven grids of ps_download_solution_fields, through the
    reference-numbered index arrays of the solver's last setup; 0 where a sample has no DOF"""
    sc = solver.scene
    sh = abi.grid_shapes(sc.nx, sc.ny, sc.nz)
    ca = solver.array("centerActiveIndices").reshape(sh["center"])
    cm = ca >= 0
    nC = int(cm.sum())
    out, off = {}, 0
    for name in ("pressure", "txx", "tyy", "tzz"):
        g = np.zeros(sh["center"], np.float64)
        g[cm] = x[off + ca[cm]]
        out[name], off = g, off + nC
    for name, grid in (("tyz", "edgeYZ"), ("txz", "edgeXZ"), ("txy", "edgeXY")):
        ea = solver.array(grid + "ActiveIndices").reshape(sh[grid])
        em = ea >= 0
        g = np.zeros(sh[grid], np.float64)
        g[em] = x[off + ea[em]]
        out[name], off = g, off + int(em.sum())
    assert off == len(x)
    return out


def gather_ref(solver, fields):
    """the inverse: the x0 a warm start gathers from carried grids through the solver's current index arrays (reference numbering)"""
    sc = solver.scene
    sh = abi.grid_shapes(sc.nx, sc.ny, sc.nz)
    parts = []
    ca = solver.array("centerActiveIndices").reshape(sh["center"])
    cm = ca >= 0
    for name in ("pressure", "txx", "tyy", "tzz"):
        v = np.zeros(int(cm.sum()), np.float64)
        v[ca[cm]] = fields[name][cm]
        parts.append(v)
    for name, grid in (("tyz", "edgeYZ"), ("txz", "edgeXZ"), ("txy", "edgeXY")):
        ea = solver.array(grid + "ActiveIndices").reshape(sh[grid])
        em = ea >= 0
        v = np.zeros(int(em.sum()), np.float64)
        v[ea[em]] = fields[name][em]
        parts.append(v)
    return np.concatenate(parts)


def _close(x, ref, tol):
    return np.linalg.norm(x - ref) <= 10 * tol * max(np.linalg.norm(ref), 1e-300)


def stirred_droplet(radius=0.33):
    """scenes.droplet with a random (seeded) face velocity: the ball at rest has b = 0 and a zero solution"""
    sc, p = scenes.droplet(24, radius=radius)
    rng = np.random.RandomState(7)
    for a in range(3):
        sc.vel[a][...] = rng.uniform(-1.0, 1.0, sc.vel[a].shape).astype(np.float32)
    return sc, p


def _it(s):
    return int(s.stats.solveData[1])


# ---- 1. the same inputs twice ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", PRECONDS)
@pytest.mark.parametrize("make", ["cavity48", "blob0"])
def test_same_inputs_twice_converge_at_once(gpu, make, precond):
    sc, p = {"cavity48": lambda: scenes.cavity(48), "blob0": lambda: scenes.blob(seed=0)}[make]()
    p.preconditioner = precond
    gpu.set_warm_start(abi.WARM_PREVIOUS_STEP)
    try:
        gpu.upload(sc, p)
        assert gpu.step_device() == abi.SUCCESS
        assert int(gpu.array("warmStartUsed")[0]) == 0                  # nothing carried yet: a cold start
        assert not gpu.array("warmStartVector").any()
        cold_it = _it(gpu)
        x1 = gpu.array("solutionVector").copy()
        assert gpu.step_device() == abi.SUCCESS
        assert int(gpu.array("warmStartUsed")[0]) == 1
        assert _it(gpu) <= 1 < cold_it, (_it(gpu), cold_it)
        assert np.array_equal(gpu.array("warmStartVector"), x1.astype(np.float32).astype(np.float64))
        x2 = gpu.array("solutionVector")
        # both solutions meet the stop rule on their TRUE residuals.  The rule bounds the residual, not the error: one step of the Chebyshev
        # polynomial (close to A^-1) from x0 also removes part of x1's own error (blob0: 2.5 % of x) — there x2 must be at least as good
        b = gpu.array("b")
        r1, r2 = b - gpu.apply(x1), b - gpu.apply(x2)
        rule = lambda r, x: min(r @ r, (r @ r) / (x @ x))
        assert rule(r2, x2) < (2 * p.tolerance) ** 2 and rule(r1, x1) < (2 * p.tolerance) ** 2
        if precond in (abi.PRE_CHEBYSHEV, abi.PRE_CHEBYSHEV_F32):
            assert np.linalg.norm(r2) <= np.linalg.norm(r1)
        else:
            assert _close(x2, x1, p.tolerance)
    finally:
        gpu.set_warm_start(abi.WARM_NONE)


# ---- 2. the geometry changes between steps ---------------------------------------------------------------------------------------------
SEQUENCES = {
    # sphere centres advanced by their collision velocity over 1.5 cells' time (up to 1.5 cells)
    "spheres32_moving": (lambda: scenes.spheres(32, tile=8), lambda: scenes.spheres(32, tile=8, t=1.5 / 32)),
    "droplet24_growing": (lambda: stirred_droplet(0.33), lambda: stirred_droplet(0.36)),
}


@pytest.mark.parametrize("precond", PRECONDS)
@pytest.mark.parametrize("seq", list(SEQUENCES))
def test_changed_geometry_starts_from_the_carried_solution(gpu, seq, precond):
    (sc1, p), (sc2, _) = SEQUENCES[seq][0](), SEQUENCES[seq][1]()
    p.preconditioner = precond
    gpu.set_warm_start(abi.WARM_PREVIOUS_STEP)
    try:
        gpu.upload(sc1, p)
        assert gpu.step_device() == abi.SUCCESS
        fields1 = gpu.solution_fields()
        gpu.upload(sc2, p)
        assert gpu.step_device() == abi.SUCCESS
        assert int(gpu.array("warmStartUsed")[0]) == 1
        it_lib, x_lib = _it(gpu), gpu.array("solutionVector").copy()
        x0 = gather_ref(gpu, fields1)
        assert np.array_equal(gpu.array("warmStartVector"), x0)
        it_np, x_np = numpy_pcg(gpu.apply, gpu.precondition, gpu.array("b"), x0, p.tolerance, p.maxSolverIterations)
        lo = max(2, 0.02 * it_np)
        hi = max(2, (0.07 if precond == abi.PRE_CHEBYSHEV_F32 else 0.02) * it_np)
        assert it_np - lo <= it_lib <= it_np + hi, (it_lib, it_np)
        assert _close(x_lib, x_np, p.tolerance)
    finally:
        gpu.set_warm_start(abi.WARM_NONE)


# ---- 3. the solution as grid fields ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", ["blob0", "droplet24", "spheres32"])
def test_solution_fields_scatter_the_solution_vector(gpu, oracle_mod, make):
    sc, p = {"blob0": lambda: scenes.blob(seed=0), "droplet24": lambda: stirred_droplet(),
             "spheres32": lambda: scenes.spheres(32, tile=8)}[make]()
    gpu.upload(sc, p)
    gpu.setup()
    with pytest.raises(Exception, match="no solve since the last setup"):
        gpu.solution_fields()
    assert gpu.solve() == abi.SUCCESS
    f = gpu.solution_fields()
    x = gpu.array("solutionVector")
    mine = scatter_ref(gpu, x)
    sh = abi.grid_shapes(sc.nx, sc.ny, sc.nz)
    for name, grid in abi.SOLUTION_FIELDS:
        assert f[name].shape == sh[grid] and f[name].dtype == np.float32
        assert np.array_equal(f[name], mine[name].astype(np.float32)), name
    assert np.abs(f["pressure"]).max() > 0
    o = oracle_mod.Oracle()
    o.run(sc, p, solve=True)
    xo = o.array("solutionVector")
    theirs = scatter_ref(gpu, xo)            # the index arrays are bit-exact between the two (test_gpu_parity)
    a = np.concatenate([f[k].ravel().astype(np.float64) for k, _ in abi.SOLUTION_FIELDS])
    b = np.concatenate([theirs[k].ravel() for k, _ in abi.SOLUTION_FIELDS])
    assert _close(a, b, p.tolerance)


def test_bad_mode_is_refused(gpu):
    import polystokes_amd
    L = polystokes_amd.lib()
    assert L.ps_set_warm_start(gpu.h, 2) == abi.INVALID
    assert "unknown mode" in L.ps_last_error(gpu.h).decode()
    assert L.ps_set_warm_start(gpu.h, -1) == abi.INVALID


# ---- 4. invalidation -------------------------------------------------------------------------------------------------------------------
def _outcome(s, rc):
    return (rc, _it(s), float(s.stats.solveData[0]).hex(), s.array("solutionVector").tobytes(), tuple(v.tobytes() for v in s.download()[0]))


def _fresh(sc, p):
    s = _new_solver()
    s.upload(sc, p)
    out = _outcome(s, s.step_device())
    s.close()
    return out


@pytest.mark.parametrize("precond", [abi.PRE_DIAGONAL, abi.PRE_CHEBYSHEV])
def test_other_grid_or_mode_zero_solves_exactly_as_a_fresh_context(gpu, precond):
    sc32, p = scenes.cavity(32, precond=precond)
    sc40, _ = scenes.cavity(40)
    gpu.set_warm_start(abi.WARM_PREVIOUS_STEP)
    try:
        gpu.upload(sc32, p)
        gpu.step_device()
        gpu.upload(sc40, p)                                  # another nx: the carried grids do not fit, the solve starts cold
        got = _outcome(gpu, gpu.step_device())
        assert int(gpu.array("warmStartUsed")[0]) == 0
        assert got == _fresh(sc40, p)
        gpu.upload(sc32, p)
        gpu.step_device()
        gpu.step_device()
        assert int(gpu.array("warmStartUsed")[0]) == 1
    finally:
        gpu.set_warm_start(abi.WARM_NONE)
    assert gpu.L.ps_query_array(gpu.h, b"warmStartVector", None) < 0        # dropped with the store
    got = _outcome(gpu, gpu.step_device())
    assert int(gpu.array("warmStartUsed")[0]) == 0
    assert got == _fresh(sc32, p)


def test_interrupted_step_leaves_the_carried_solution_alone(gpu):
    sc1, p = stirred_droplet(0.33)
    sc2, _ = stirred_droplet(0.36)
    p.tolerance = 1e-6
    gpu.set_warm_start(abi.WARM_PREVIOUS_STEP)
    try:
        gpu.upload(sc1, p)
        assert gpu.step_device() == abi.SUCCESS
        gpu.upload(sc2, p)
        gpu.set_interrupt(lambda: True)
        try:
            assert gpu.step_device() == abi.INCOMPLETE
        finally:
            gpu.set_interrupt(None)
        assert int(gpu.array("warmStartUsed")[0]) == 1
        v_interrupted = gpu.array("warmStartVector").copy()
        assert gpu.step_device() == abi.SUCCESS
        assert np.array_equal(gpu.array("warmStartVector"), v_interrupted)
        gpu.step_device()                                    # the kept step above did carry: now the start is its solution
        assert not np.array_equal(gpu.array("warmStartVector"), v_interrupted)
    finally:
        gpu.set_warm_start(abi.WARM_NONE)


# ---- 5. memory ---------------------------------------------------------------------------------------------------------------------
def test_carried_state_is_flat_across_steps_and_released_when_dropped():
    s = _new_solver()
    sc, p = scenes.cavity(48, precond=abi.PRE_DIAGONAL)
    s.upload(sc, p)
    s.step_device()
    s.step_device()
    n = len(s.array("solutionVector"))                       # (reading an fp64 array allocates its staging buffer once)
    base = s.memory_stats()["live_bytes"]
    s.set_warm_start(abi.WARM_PREVIOUS_STEP)
    seen = []
    for _ in range(4):
        assert s.step_device() == abi.SUCCESS
        m = s.memory_stats()
        assert m["deferred_bytes"] == 0
        seen.append(m["live_bytes"])
    assert len(set(seen)) == 1, seen
    samples = 4 * sc.nx * sc.ny * sc.nz + sum(int(np.prod(abi.grid_shapes(sc.nx, sc.ny, sc.nz)[g])) for g in ("edgeYZ", "edgeXZ", "edgeXY"))
    assert seen[0] - base == 4 * samples + 8 * n, (seen[0] - base, samples, n)
    s.set_warm_start(abi.WARM_NONE)
    m = s.memory_stats()
    assert m["deferred_bytes"] == 0 and m["live_bytes"] == base
    s.close()


# ---- 6. both step forms, fallback formats, the release library -------------------------------------------------------------------------
_CHILD = (
    "n, precond = int(sys.argv[1]), int(sys.argv[2])\n"
    "sc, p = scenes.cavity(n, precond=precond)\n"
    "s = polystokes_amd.Solver(0)\n"
    "s.set_warm_start(1)\n"
    "s.upload(sc, p)\n"
    "rc1 = s.step_device(); it1 = int(s.stats.solveData[1]); x1 = s.array('solutionVector').copy()\n"
    "rc2 = s.step_device(); it2 = int(s.stats.solveData[1]); x2 = s.array('solutionVector')\n"
    "out = dict(rc=[rc1, rc2], it=[it1, it2], used=int(s.array('warmStartUsed')[0]), fused=int(s.array('fusedStep')[0]),\n"
    "           x0_exact=bool(np.array_equal(s.array('warmStartVector'), x1.astype(np.float32).astype(np.float64))),\n"
    "           dx=float(np.linalg.norm(x2 - x1) / np.linalg.norm(x1)), values_coded=int(s.array('valuesCoded')[0]))\n"
    "s.close()\n"
    "print('RESULT ' + json.dumps(out))\n"
)


@pytest.mark.parametrize("n,precond,env", [
    (80, abi.PRE_DIAGONAL, {}),                                    # 1.56 M rows: the four-kernel step
    (80, abi.PRE_CHEBYSHEV_F32, {}),
    (80, abi.PRE_DIAGONAL, {"PS_FUSED_R": "0"}),                   # the five-kernel step at the same size
    (80, abi.PRE_CHEBYSHEV, {"PS_FUSED_R": "0"}),
    (32, abi.PRE_CHEBYSHEV, {"PS_COL32": "1"}),                    # fallback storage formats
    (32, abi.PRE_DIAGONAL, {"PS_FORCE_FP64_VALUES": "1"}),
    (32, abi.PRE_IDENTITY, {"PS_LIB": os.path.join(ROOT, "polystokes_amd", "libpolystokes_hip_release.so")}),
])
def test_step_forms_fallbacks_and_release_library(n, precond, env):
    r = children.run_python(_CHILD, n, int(precond), limit=600, env=env).result()
    assert r["rc"] == [abi.SUCCESS, abi.SUCCESS]
    assert r["used"] == 1 and r["x0_exact"]
    assert r["it"][1] <= 1 < r["it"][0], r["it"]
    assert r["dx"] <= 10 * 1e-3
    if n == 80:
        assert r["fused"] == (0 if env.get("PS_FUSED_R") == "0" else 1)
    else:
        assert r["fused"] == 0
    if "PS_FORCE_FP64_VALUES" in env:
        assert r["values_coded"] == 0


# ---- 7. decompositions start cold ------------------------------------------------------------------------------------------------------
def test_in_process_group_ignores_the_mode():
    import polystokes_amd
    sc, p = scenes.cavity(32, tile=8, precond=abi.PRE_DIAGONAL)
    results = []
    for mode in (abi.WARM_NONE, abi.WARM_PREVIOUS_STEP):
        grp = polystokes_amd.Group(2)
        for r in grp.ranks:
            r.set_warm_start(mode)
        steps = []
        for _ in range(2):
            assert grp.solve_scene(sc, p) == abi.SUCCESS
            assert all(int(r.array("warmStartUsed")[0]) == 0 for r in grp.ranks)
            steps.append((int(grp.stats.solveData[1]), tuple(v.tobytes() for v in grp.vel)))
        results.append(steps)
        grp.close()
    assert results[0] == results[1]

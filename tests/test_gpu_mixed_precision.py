"""Mixed-precision PCG (ps_set_solve_precision) on the GPU: fp32 Krylov vectors in passes around the fp64 x, the stop rule decided on the
fp64 residual b - A x (include/polystokes.h; the scheme restated in numpy: mixed_precision_ref.py, its caps checked on the oracle's
operator by test_mixed_precision_ref_cpu.py).

The reference of every case is the fp64 mode of the same library: iterations against mode 0 on the same context, the error against a mode-0
solve at tol 1e-12.  Two valid solves stop at different iterates, so x is never compared with x64 directly.
Every case prints its figures before it asserts (run with -s); profiles/mixed_precision.md says which of them have been measured."""
import math
import os

import numpy as np
import pytest

from polystokes_amd import _abi as abi
from polystokes_amd import scenes

import children
from helpers import fdot
from mixed_precision_ref import ERROR_CAP, ITERATION_CAP, PASS_CAP

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP64, MIXED = abi.PRECISION_FP64, abi.PRECISION_MIXED
SCENES = {"blob0": lambda: scenes.blob(seed=0), "cavity32": lambda: scenes.cavity(32), "spheres32": lambda: scenes.spheres(32, tile=8)}
PRECONDS = {"identity": abi.PRE_IDENTITY, "jacobi": abi.PRE_DIAGONAL}
MAXIT = 20000


def _new_solver():
    import polystokes_amd
    return polystokes_amd.Solver(0)


@pytest.fixture(scope="module")
def gpu():
    s = _new_solver()
    yield s
    s.set_solve_precision(FP64)
    s.close()


def _case(scene, pre, tol, make=None):
    sc, p = make() if make else SCENES[scene]() if isinstance(scene, str) else scene
    p.preconditioner = PRECONDS[pre] if isinstance(pre, str) else pre
    p.tolerance = tol
    p.maxSolverIterations = MAXIT
    return sc, p


def _it(s):
    return int(s.stats.solveData[1])


def _used(s):
    return int(s.array("solvePrecisionUsed")[0])


def _rule(s, x):
    """min(r.r, r.r / x.x) of r = b - A x through the library's fp64 operator, with correctly rounded sums"""
    r = s.array("b") - s.apply(x)
    rr, xx = fdot(r, r), fdot(x, x)
    return min(rr, rr / xx) if xx > 0 else rr


def _solve(s, sc, p, mode):
    assert s.set_solve_precision(mode) == abi.SUCCESS
    s.upload(sc, p)
    return s.step_device()


def check_mixed_solve(s, p, it64, label=""):
    """the assertions every mixed solve meets: mixed throughout, the rule on the true residual, the reported value, iterations, passes"""
    tol = p.tolerance
    assert _used(s) == 1
    passes = [int(v) for v in s.array("solvePassIterations")]
    x = s.array("solutionVector")
    rule = _rule(s, x)
    reported = float(s.array("solveTrueResidual")[0])
    print("%s tol %g: fp64 %d -> mixed %d / %d passes %s (ratio %.4f), rule / tol^2 %.4f" %
          (label, tol, it64, sum(passes), len(passes), passes, sum(passes) / max(it64, 1), rule / tol ** 2))
    assert rule < tol * tol * (1 + 1e-9), (rule, tol * tol)
    assert abs(reported - math.sqrt(rule)) <= 1e-9 * math.sqrt(rule), (reported, math.sqrt(rule))
    assert float(s.stats.solveData[0]) == reported and _it(s) == sum(passes)
    assert sum(passes) <= ITERATION_CAP(it64), (passes, it64)
    assert 1 <= len(passes) <= PASS_CAP, passes
    return x


# ---- 1. the main check ---------------------------------------------------------------------------------------------------------------
_xstar = {}


def xstar(s, scene, pre, make=None):
    """the mode-0 solve at tol 1e-12, once per system"""
    if (scene, pre) not in _xstar:
        sc, p = _case(scene, pre, 1e-12, make)
        assert _solve(s, sc, p, FP64) == abi.SUCCESS
        _xstar[(scene, pre)] = s.array("solutionVector").copy()
    return _xstar[(scene, pre)]


@pytest.mark.parametrize("tol", [1e-3, 1e-6, 1e-8])
@pytest.mark.parametrize("pre", list(PRECONDS))
@pytest.mark.parametrize("scene", list(SCENES))
def test_mixed_solve_meets_the_rule_and_the_caps(gpu, scene, pre, tol):
    mixed_solve_meets_the_rule_and_the_caps(gpu, scene, pre, tol)


def mixed_solve_meets_the_rule_and_the_caps(gpu, scene, pre, tol, make=None):
    """scene: a name in SCENES, or any name with `make`, the function that builds (scene, params) (test_gpu_vector_tails.py)"""
    xs = xstar(gpu, scene, pre, make)
    sc, p = _case(scene, pre, tol, make)
    assert _solve(gpu, sc, p, FP64) == abi.SUCCESS
    assert _used(gpu) == 0
    with pytest.raises(KeyError):
        gpu.array("solvePassIterations")
    it64, x64 = _it(gpu), gpu.array("solutionVector").copy()
    assert _solve(gpu, sc, p, MIXED) == abi.SUCCESS
    x = check_mixed_solve(gpu, p, it64, "%s %s" % (scene, pre))
    e, e64 = np.linalg.norm(x - xs), np.linalg.norm(x64 - xs)
    print("    error ratio %.3f" % (e / e64))
    assert e <= ERROR_CAP * e64, (e, e64)


# ---- 2. both step forms and the release library, in child processes (the switches are read once per process) ----------------------------
_CHILD = (
    "from helpers import fdot\n"
    "n, precond, tol = int(sys.argv[1]), int(sys.argv[2]), float(sys.argv[3])\n"
    "tile = int(sys.argv[4]) if len(sys.argv) > 4 else 16\n"
    "sc, p = scenes.cavity(n, tile=tile, precond=precond)\n"
    "p.tolerance = tol; p.maxSolverIterations = 20000\n"
    "def outcome(s, rc):\n"
    "    return [rc, int(s.stats.solveData[1]), float(s.stats.solveData[0]).hex(), s.array('solutionVector').tobytes().hex(),\n"
    "            [v.tobytes().hex() for v in s.download()[0]]]\n"
    "f = polystokes_amd.Solver(0)\n"
    "f.upload(sc, p); fresh = outcome(f, f.step_device()); it64 = int(f.stats.solveData[1]); f.close()\n"
    "s = polystokes_amd.Solver(0)\n"
    "s.set_solve_precision(1)\n"
    "s.upload(sc, p); rc = s.step_device(); got = outcome(s, rc)\n"
    "used = int(s.array('solvePrecisionUsed')[0])\n"
    "x = s.array('solutionVector'); r = s.array('b') - s.apply(x); rr, xx = fdot(r, r), fdot(x, x)\n"
    "out = dict(rc=rc, used=used, it64=it64, fused=int(s.array('fusedStep')[0]), rule=min(rr, rr / xx), same=bool(got == fresh),\n"
    "           passes=[int(v) for v in s.array('solvePassIterations')] if used else [],\n"
    "           reported=float(s.array('solveTrueResidual')[0]) if used else None, it=int(s.stats.solveData[1]),\n"
    "           values_coded=int(s.array('valuesCoded')[0]), columns16=int(s.array('columns16')[0]), row_per_lane=int(s.array('rowPerLane')[0]))\n"
    "s.close()\n"
    "print('RESULT ' + json.dumps(out))\n"
)


def _child(n, precond, tol, env, tile=16):
    return children.run_python(_CHILD, n, int(precond), repr(tol), tile, limit=600, env=env).result()


@pytest.mark.parametrize("n,env,fused", [
    (80, {}, 1),                                                   # 1.56 M rows: the four-kernel step by default
    (80, {"PS_FUSED_R": "0"}, 0),                                  # the five-kernel step at the same size (A p stored as fp32)
    (32, {"PS_FUSED_R": "1"}, 1),                                  # the four-kernel step on a small system
    (32, {"PS_LIB": os.path.join(ROOT, "polystokes_amd", "libpolystokes_hip_release.so")}, 0),
])
def test_step_forms_and_release_library(n, env, fused):
    tol = 1e-6
    r = _child(n, abi.PRE_DIAGONAL, tol, env)
    print(r["it64"], r["passes"], r["rule"] / tol ** 2)
    assert r["rc"] == abi.SUCCESS and r["used"] == 1 and r["fused"] == fused, r
    assert r["rule"] < tol * tol * (1 + 1e-9)
    assert abs(r["reported"] - math.sqrt(r["rule"])) <= 1e-9 * math.sqrt(r["rule"])
    assert r["it"] == sum(r["passes"]) <= ITERATION_CAP(r["it64"]), (r["passes"], r["it64"])
    assert 1 <= len(r["passes"]) <= PASS_CAP


# ---- 3. the two diagonals as fp64 fields -------------------------------------------------------------------------------------------------
def _viscosity_field_cavity():
    sc, p = scenes.cavity(32, precond=abi.PRE_DIAGONAL)
    z, y, x = np.meshgrid(*[(np.arange(32) + 0.5) / 32] * 3, indexing="ij")
    sc.viscosity[...] = (1.5 + np.sin(9 * x + 0.2) * np.cos(8 * z - 0.4) + 0.3 * np.sin(7 * y)).astype(np.float32)
    return sc, p


@pytest.mark.parametrize("field", ["viscosity", "viscosity+density"])
def test_field_diagonals(gpu, field):
    sc, p = _viscosity_field_cavity()
    if field.endswith("density"):
        scenes.with_density_field(sc, "smooth", rho0=100.0)
    sc, p = _case((sc, p), abi.PRE_DIAGONAL, 1e-6)
    assert _solve(gpu, sc, p, FP64) == abi.SUCCESS
    it64 = _it(gpu)
    assert _solve(gpu, sc, p, MIXED) == abi.SUCCESS
    assert int(gpu.array("diagonalsCoded")[0]) & 1 == 0             # the stress diagonal is the fp64 array (k_spmv_St_ell2 with UC = false)
    if field.endswith("density"):
        assert int(gpu.array("densityField")[0]) == 1 and int(gpu.array("diagonalsCoded")[0]) & 2 == 0    # ... and the face mass (k_spmv_S_ell2u)
    check_mixed_solve(gpu, p, it64, field)


# ---- 4. everywhere else the solve is the fp64 one, byte for byte ---------------------------------------------------------------------------
def _outcome(s, rc):
    return (rc, _it(s), float(s.stats.solveData[0]).hex(), s.array("solutionVector").tobytes(), tuple(v.tobytes() for v in s.download()[0]))


def _fresh(sc, p):
    s = _new_solver()
    s.upload(sc, p)
    out = _outcome(s, s.step_device())
    s.close()
    return out


@pytest.mark.parametrize("what", ["chebyshev", "chebyshev_f32", "eigen"])
def test_other_solvers_ignore_the_mode(gpu, what):
    sc, p = scenes.cavity(32, precond={"chebyshev": abi.PRE_CHEBYSHEV, "chebyshev_f32": abi.PRE_CHEBYSHEV_F32, "eigen": abi.PRE_DIAGONAL}[what])
    if what == "eigen":
        p.solverType = abi.EIGEN
    got = _outcome(gpu, _solve(gpu, sc, p, MIXED))
    assert _used(gpu) == 0
    assert got[0] == abi.SUCCESS and got == _fresh(sc, p)


def test_in_process_group_ignores_the_mode():
    import polystokes_amd
    sc, p = scenes.cavity(32, tile=8, precond=abi.PRE_DIAGONAL)
    results = []
    for mode in (FP64, MIXED):
        grp = polystokes_amd.Group(2)
        assert grp.set_solve_precision(mode) == abi.SUCCESS
        assert grp.solve_scene(sc, p) == abi.SUCCESS
        assert all(_used(r) == 0 for r in grp.ranks)
        results.append((int(grp.stats.solveData[1]), float(grp.stats.solveData[0]).hex(), tuple(r.array("solutionVector").tobytes() for r in grp.ranks),
                        tuple(v.tobytes() for v in grp.vel)))
        grp.close()
    assert results[0] == results[1]


@pytest.mark.parametrize("env,flag", [({"PS_FORCE_FP64_VALUES": "1"}, "values_coded"), ({"PS_COL32": "1"}, "columns16"), ({"PS_NO_ELL": "1"}, "row_per_lane")])
def test_fallback_formats_ignore_the_mode(env, flag):
    r = _child(32, abi.PRE_DIAGONAL, 1e-6, env)
    assert r[flag] == 0, r[flag]                                   # the format the switch forces is the one that ran
    assert r["rc"] == abi.SUCCESS and r["used"] == 0 and r["same"]


# ---- 5. mode 0 is untouched ------------------------------------------------------------------------------------------------------------
def test_mode_zero_after_mixed_solves_exactly_as_a_fresh_context(gpu):
    sc, p = _case("cavity32", "jacobi", 1e-6)
    assert _solve(gpu, sc, p, MIXED) == abi.SUCCESS and _used(gpu) == 1
    got = _outcome(gpu, _solve(gpu, sc, p, FP64))
    assert _used(gpu) == 0
    assert got == _fresh(sc, p)


def test_memory_is_flat_and_released_with_the_mode():
    s = _new_solver()
    sc, p = _case("cavity32", "jacobi", 1e-6)
    s.upload(sc, p)
    s.step_device()
    s.step_device()
    n = len(s.array("solutionVector"))                             # (reading an fp64 array allocates its staging buffer once)
    rows = s.nA + len(s.array("reducedRowFace"))           # the face rows of S: active and skin rows
    base = s.memory_stats()["live_bytes"]
    assert s.set_solve_precision(MIXED) == abi.SUCCESS
    assert s.memory_stats()["live_bytes"] == base                  # the setting alone allocates nothing
    seen = []
    for _ in range(4):
        assert s.step_device() == abi.SUCCESS and _used(s) == 1
        m = s.memory_stats()
        assert m["deferred_bytes"] == 0
        seen.append(m["live_bytes"])
    assert len(set(seen)) == 1, seen
    # d, p, r and (five-kernel step, as here) A p at 4 B per DOF, t at 4 B per face row (+ 1)
    assert int(s.array("fusedStep")[0]) == 0
    assert seen[0] - base == 4 * 4 * n + 4 * (rows + 1), (seen[0] - base, n, rows)
    assert s.set_solve_precision(FP64) == abi.SUCCESS
    m = s.memory_stats()
    assert m["deferred_bytes"] == 0 and m["live_bytes"] == base
    s.close()


def test_bad_mode_is_refused_and_keeps_the_setting(gpu):
    assert gpu.set_solve_precision(MIXED) == abi.SUCCESS
    for bad in (2, -1, 7):
        assert gpu.L.ps_set_solve_precision(gpu.h, bad) == abi.INVALID
        assert "unknown mode" in gpu.last_error()
    sc, p = _case("blob0", "jacobi", 1e-3)
    gpu.upload(sc, p)
    assert gpu.step_device() == abi.SUCCESS and _used(gpu) == 1   # the previous setting held
    assert gpu.set_solve_precision(FP64) == abi.SUCCESS


# ---- 6. composition ---------------------------------------------------------------------------------------------------------------------
def test_warm_start_is_a_first_pass_from_the_carried_solution(gpu):
    sc, p = _case("cavity32", "jacobi", 1e-6)
    gpu.set_warm_start(abi.WARM_PREVIOUS_STEP)
    try:
        assert _solve(gpu, sc, p, MIXED) == abi.SUCCESS
        assert _used(gpu) == 1 and int(gpu.array("warmStartUsed")[0]) == 0
        cold = _it(gpu)
        assert gpu.step_device() == abi.SUCCESS
        assert _used(gpu) == 1 and int(gpu.array("warmStartUsed")[0]) == 1
        assert _it(gpu) <= 2 < cold, (_it(gpu), cold)
        assert _rule(gpu, gpu.array("solutionVector")) < p.tolerance ** 2 * (1 + 1e-9)
    finally:
        gpu.set_warm_start(abi.WARM_NONE)
        gpu.set_solve_precision(FP64)


def test_picard_passes_run_mixed():
    s = _new_solver()
    try:
        assert s.set_rheology(flow_index=0.7, passes=2, min_shear_rate=1e-2, min_viscosity=1e-3, max_viscosity=1e5) == abi.SUCCESS
        assert s.set_solve_precision(MIXED) == abi.SUCCESS
        sc, p = scenes.blob()
        p.preconditioner = abi.PRE_DIAGONAL
        assert s.step(sc, p) == abi.SUCCESS
        it = list(s.array("rheologyIterations"))
        assert len(it) == 3, it
        assert _used(s) == 1 and int(s.array("warmStartUsed")[0]) == 1      # the last pass started from the one before
        assert it[-1] == sum(int(v) for v in s.array("solvePassIterations"))
    finally:
        s.close()


def test_interrupt_leaves_the_input_velocity(gpu):
    sc, p = _case("spheres32", "jacobi", 1e-8)
    gpu.set_solve_precision(MIXED)
    gpu.set_interrupt(lambda: True)
    try:
        assert gpu.step(sc, p) == abi.INCOMPLETE
    finally:
        gpu.set_interrupt(None)
        gpu.set_solve_precision(FP64)
    assert _used(gpu) == 1 and _it(gpu) == 25                      # stopped at the first batch end of the first pass
    for q in range(3):
        assert gpu.vel[q].tobytes() == sc.vel[q].tobytes()


def test_budget_runs_out_into_the_same_bicgstab(gpu):
    sc, p = _case("spheres32", "jacobi", 1e-8)
    p.maxSolverIterations = 5
    rc64 = _solve(gpu, sc, p, FP64)
    assert gpu.stats.usedBiCGStab == 1
    x64 = gpu.array("solutionVector").tobytes()
    rc = _solve(gpu, sc, p, MIXED)
    try:
        assert rc == rc64 and gpu.stats.usedBiCGStab == 1
        assert _used(gpu) == 1 and list(gpu.array("solvePassIterations")) == [5]
        assert gpu.array("solutionVector").tobytes() == x64         # BiCGStab starts from zero either way
    finally:
        gpu.set_solve_precision(FP64)


# ---- 7. determinism ---------------------------------------------------------------------------------------------------------------------
def test_two_mixed_solves_are_identical(gpu):
    sc, p = _case("cavity32", "jacobi", 1e-6)
    try:
        assert _solve(gpu, sc, p, MIXED) == abi.SUCCESS
        first = (_it(gpu), list(gpu.array("solvePassIterations")), gpu.array("solutionVector").tobytes())
        assert _solve(gpu, sc, p, MIXED) == abi.SUCCESS
        assert (_it(gpu), list(gpu.array("solvePassIterations")), gpu.array("solutionVector").tobytes()) == first
    finally:
        gpu.set_solve_precision(FP64)

"""The mixed-precision PCG scheme (mixed_precision_ref.mixed_pcg) on the oracle's operator, without a GPU: the caps that
test_gpu_mixed_precision.py asserts on the device — the stop rule on the true residual, the iterations against the fp64 solve, the number of
passes, the error against a solve at 1e-12 — asserted on the algorithm alone, so that a cap the algorithm cannot meet is found here.

Measured here (iterations: index of the fp64 solve's converged iteration -> sum of the iterations the passes ran / passes; the error ratio
||x - x*|| / ||x64 - x*||):
  blob0    identity  1e-3 30 -> 31 / 1, 1.00    1e-6 123 -> 126 / 2, 1.04   1e-8 237 -> 236 / 2, 1.57
  blob0    Jacobi    1e-3 21 -> 22 / 1, 1.00    1e-6  94 ->  98 / 2, 0.99   1e-8 147 -> 154 / 2, 0.82
  cavity32 Jacobi    1e-3 111 -> 111 / 2, 1.19  1e-6 265 -> 280 / 2, 0.65
(a pass counts the iterations it ran; the fp64 solve reports the index of the iteration that met the rule, one less)"""
import numpy as np
import pytest

from polystokes_amd import _abi as abi
from polystokes_amd import scenes

import mixed_precision_ref as ref

SCENES = {"blob0": lambda: scenes.blob(seed=0), "cavity32": lambda: scenes.cavity(32)}
CASES = [("blob0", pre, tol) for pre in ("identity", "jacobi") for tol in (1e-3, 1e-6, 1e-8)] + [("cavity32", "jacobi", 1e-3), ("cavity32", "jacobi", 1e-6)]
MAXIT = 20000
_systems = {}


def system(oracle_mod, scene, pre):
    """(A, M, b, x*) of a scene and preconditioner, built once: x* is the fp64 solve at tol 1e-12"""
    key = (scene, pre)
    if key not in _systems:
        sc, p = SCENES[scene]()
        p.preconditioner = abi.PRE_IDENTITY if pre == "identity" else abi.PRE_DIAGONAL
        p.tolerance = 1e-12
        p.maxSolverIterations = MAXIT
        o = oracle_mod.Oracle()
        o.run(sc, p, solve=False)
        b = o.array("b").copy()
        M = (lambda r: np.array(r, copy=True)) if pre == "identity" else o.precondition
        _, xstar = ref.fp64_pcg(o.apply, M, b, 1e-12, MAXIT)
        _systems[key] = (o, o.apply, M, b, xstar)
    return _systems[key][1:]


@pytest.mark.parametrize("scene,pre,tol", CASES)
def test_scheme_meets_the_caps_on_the_oracle_operator(oracle_mod, scene, pre, tol):
    A, M, b, xstar = system(oracle_mod, scene, pre)
    it64, x64 = ref.fp64_pcg(A, M, b, tol, MAXIT)
    out = ref.mixed_pcg(A, M, b, None, tol, MAXIT)
    x = out["x"]
    ratio = np.linalg.norm(x - xstar) / np.linalg.norm(x64 - xstar)
    print("%s %s %g: fp64 %d -> mixed %d / %d passes %s, error ratio %.3f, rule / tol^2 %.3f" %
          (scene, pre, tol, it64, sum(out["passes"]), len(out["passes"]), out["passes"], ratio, ref.rule(b - A(x), x) / tol ** 2))
    assert out["status"] == "success"
    assert ref.rule(b - A(x), x) < tol * tol                       # the rule on the true fp64 residual
    assert out["rre"] == ref.rule(b - A(x), x)                     # ... is what the scheme decided on
    assert sum(out["passes"]) <= ref.ITERATION_CAP(it64), (out["passes"], it64)
    assert len(out["passes"]) <= ref.PASS_CAP
    assert ratio <= ref.ERROR_CAP


def test_warm_start_is_a_first_pass_with_x(oracle_mod):
    """a carried x0 (the fp32-rounded solution, as the warm-start grids hold it): the rule uses x0 . x0 frozen, and the solve takes a
    couple of iterations"""
    A, M, b, _ = system(oracle_mod, "blob0", "jacobi")
    tol = 1e-6
    _, x64 = ref.fp64_pcg(A, M, b, tol, MAXIT)
    out = ref.mixed_pcg(A, M, b, ref.f32(x64), tol, MAXIT)
    assert out["status"] == "success" and sum(out["passes"]) <= 2, out["passes"]
    assert ref.rule(b - A(out["x"]), out["x"]) < tol * tol


def test_budget_is_one_over_all_passes(oracle_mod):
    A, M, b, _ = system(oracle_mod, "blob0", "identity")
    out = ref.mixed_pcg(A, M, b, None, 1e-8, 100)                  # the first pass alone would take more
    assert out["status"] == "maxit" and sum(out["passes"]) == 100


def test_a_tolerance_below_fp32_stagnates_into_the_fp64_solve(oracle_mod):
    """at 1e-14 the passes stop gaining before the rule is met: the scheme reports it (the library then continues in fp64) and never claims success"""
    A, M, b, _ = system(oracle_mod, "blob0", "jacobi")
    out = ref.mixed_pcg(A, M, b, None, 1e-14, MAXIT)
    assert out["status"] in ("success", "stagnated")
    if out["status"] == "success":
        assert ref.rule(b - A(out["x"]), out["x"]) < 1e-28
    assert len(out["passes"]) <= ref.MAX_PASSES

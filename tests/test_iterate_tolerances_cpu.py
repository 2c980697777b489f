"""The reference PCG driver of tests/test_gpu_iterates.py on the CPU oracle: it reproduces the oracle's own solve, and every bound on the
distance between a device iterate and it is tight enough to see a wrong step — the reference itself, perturbed in one of two ways, must land
further away than the bound:
  - beta of the 24th iteration (the one the 25th step uses) scaled by 1 + 1e-6,
  - z = M^-1 r with one row zeroed in every iteration.
The fp32 polynomial's bound (ITERATE_BOUND_F32) sits above what the beta perturbation moves (1e-9 to 5e-8 relative): there only the zeroed
row is checked."""
import numpy as np
import pytest

from polystokes_amd import _abi as abi
from polystokes_amd import scenes

from helpers import CG_BATCH, ITERATE_BOUND, ITERATE_BOUND_F32, ITERATE_SHORT, numpy_pcg, relerr, trajectory_params
from test_gpu_iterates import all_cases, make_case

SCENES = {
    "cavity32": lambda: scenes.cavity(32),
    "coil32": lambda: scenes.coil(32, tile=8),
    "spheres32": lambda: scenes.spheres(32, tile=8),
    "blob6": lambda: scenes.blob(seed=6),
}


def _oracle(oracle_mod, scene, precond, degree=4, solve=False):
    sc, p = SCENES[scene]()
    p.preconditioner = precond
    p.preconditionerDegree = degree
    o = oracle_mod.Oracle()
    o.run(sc, p if solve else trajectory_params(p), solve=solve)
    M = o.precondition if precond != abi.PRE_IDENTITY else (lambda r: np.array(r, copy=True))
    return o, p, M


@pytest.mark.parametrize("scene,precond", [("blob6", abi.PRE_DIAGONAL), ("coil32", abi.PRE_CHEBYSHEV)])
def test_reference_driver_reproduces_the_oracle_solve(oracle_mod, scene, precond):
    """the oracle's converged iteration count exactly, and its x; stopped after that many iterations the driver gives the same x"""
    o, p, M = _oracle(oracle_mod, scene, precond, degree=2, solve=True)
    b = o.array("b")
    ito, xo = int(o.stats.solveData[1]), o.array("solutionVector")
    it, x = numpy_pcg(o.apply, M, b, np.zeros(len(b)), p.tolerance, p.maxSolverIterations)
    assert it == ito
    assert relerr(x, xo) <= 1e-11
    k, xs = numpy_pcg(o.apply, M, b, np.zeros(len(b)), p.tolerance, p.maxSolverIterations, iters=ito + 1)
    assert k == ito + 1 and np.array_equal(xs, x)


@pytest.mark.parametrize("scene,pre", all_cases())
def test_bounds_reject_a_perturbed_reference(oracle_mod, scene, pre):
    """every case test_gpu_iterates.py compares, at the iterates it compares"""
    sc, p = make_case(scene, pre)
    precond = p.preconditioner
    o = oracle_mod.Oracle()
    o.run(sc, trajectory_params(p), solve=False)
    M = o.precondition if precond != abi.PRE_IDENTITY else (lambda r: np.array(r, copy=True))
    b = o.array("b")
    n = len(b)
    ks = tuple(CG_BATCH * m for m in ITERATE_SHORT.get((scene, pre), (1, 2)))
    bnd = ITERATE_BOUND_F32 if precond == abi.PRE_CHEBYSHEV_F32 else ITERATE_BOUND

    def run(A, Mf, **kw):
        xs = {}
        numpy_pcg(A, Mf, b, np.zeros(n), 0.0, 0, iters=ks[-1], on_iterate=lambda k, x: xs.__setitem__(k, x.copy()) if k in ks else None, **kw)
        return xs

    ref = run(o.apply, M)
    beta = run(o.apply, M, beta_scale=lambda i, bt: bt * (1 + 1e-6) if i == CG_BATCH - 2 else bt)
    row = n // 3

    def m_skip(r):
        z = M(r)
        z[row] = 0.0
        return z

    skip = run(o.apply, m_skip)
    for k in ks:
        if precond != abi.PRE_CHEBYSHEV_F32:
            assert relerr(beta[k], ref[k]) > bnd, (k, relerr(beta[k], ref[k]), bnd)
        assert relerr(skip[k], ref[k]) > bnd, (k, relerr(skip[k], ref[k]), bnd)

"""The PCG iterate after exactly 25 and 50 iterations against a plain fp64 restatement (helpers.numpy_pcg, fsum dot products) on the oracle's
operator and preconditioner.

A converged answer cannot see a wrong step kernel: PCG corrects itself and only takes a few more iterations.  The iterate after a fixed number
of iterations can: an interrupt (ps_set_interrupt) stops the solve at the m-th batch boundary, where solutionVector holds x after 25 m
iterations.  x_50 crosses one batch boundary, where the parity of the double-buffered scalars (CG_BATCH = 25 is odd) flips.

Bounds: ITERATE_BOUND (fp64 steps) and ITERATE_BOUND_F32 (the fp32 Chebyshev polynomial, its M taken from the device) in helpers.py, measured on
an MI355X and checked against two perturbations of the reference itself by test_iterate_tolerances_cpu.py."""
import json

import numpy as np
import pytest

from polystokes_amd import _abi as abi
from polystokes_amd import scenes

import children
from helpers import CG_BATCH, ITERATE_BOUND, ITERATE_BOUND_F32, ITERATE_DROPPED, ITERATE_SHORT, iterate_after, numpy_pcg, relerr, trajectory_params

pytestmark = pytest.mark.gpu


SCENES = {
    "cavity32": lambda: scenes.cavity(32),
    "coil32": lambda: scenes.coil(32, tile=8),
    "spheres32": lambda: scenes.spheres(32, tile=8),
    "blob6": lambda: scenes.blob(seed=6),                  # a viscosity field
    # the walk-forcing sets: S and St have more than 224 pairs of chunks (301 and 537 on spheres48), so that on a grid of 64 the runs of
    # 32 pairs dealt to every XCD hold chunks for every workgroup (coil48's S has 152 pairs: XCDs 5-7 would get none)
    "cavity48": lambda: scenes.cavity(48, tile=8),
    "coil48": lambda: scenes.coil(48, tile=8),
    "spheres48": lambda: scenes.spheres(48, tile=8),
    # the vector kernels' scalar tails (test_gpu_vector_tails.py): nSystem % 4 = 1, 2, 3 (viscosity fields: the fp64 stress diagonal) and 1 (the coded one)
    "tail1": lambda: scenes.blob(20, 18, 22, seed=4, tile=8),
    "tail2": lambda: scenes.blob(20, 18, 22, seed=1, tile=8),
    "tail3": lambda: scenes.blob(20, 18, 22, seed=2, tile=8),
    "tail1c": lambda: scenes.coil(30, tile=8),
}
PRECONDS = {"identity": (abi.PRE_IDENTITY, 0), "jacobi": (abi.PRE_DIAGONAL, 0), "cheb1": (abi.PRE_CHEBYSHEV, 1), "cheb2": (abi.PRE_CHEBYSHEV, 2),
            "cheb4": (abi.PRE_CHEBYSHEV, 4), "cheb10": (abi.PRE_CHEBYSHEV, 10), "cheb32": (abi.PRE_CHEBYSHEV_F32, 4)}


def make_case(scene, pre):
    sc, p = SCENES[scene]()
    p.preconditioner, deg = PRECONDS[pre]
    if deg:
        p.preconditionerDegree = deg
    return sc, p


def _identity(r):
    return np.array(r, copy=True)


def run_case(scene, pre, batches=None, ops=False):
    """One single-domain case on a fresh context: the device iterates after 25 m iterations (m in batches) against the reference.
    Returns {"drift": {iterations: relerr}, "fused", "apply", "precondition" (ops: full-vector relative errors against the oracle),
    "walk" (the launchWalk records of the last solve)}."""
    import polystokes_amd
    from oracle import ps_oracle
    sc, p = make_case(scene, pre)
    if batches is None:
        batches = ITERATE_SHORT.get((scene, pre), (1, 2))
    gpu = polystokes_amd.Solver(0)
    try:
        got = {CG_BATCH * m: iterate_after(gpu, m, sc, p) for m in batches}
        out = {"fused": int(gpu.array("fusedStep")[0]), "walk": gpu.array("launchWalk").reshape(5, 8).tolist()}
        b = gpu.array("b")
        n = len(b)
        o = ps_oracle.Oracle()
        o.run(sc, trajectory_params(p), solve=False)
        A, M = o.apply, o.precondition
        if ops:
            rng = np.random.RandomState(5)
            w = rng.standard_normal(n)
            out["apply"] = relerr(gpu.apply(w), o.apply(w))
            r = rng.standard_normal(n)
            out["precondition"] = relerr(gpu.precondition(r), o.precondition(r))
        if pre == "identity":
            M = _identity
        elif pre == "cheb32":
            M = gpu.precondition            # the fp32 polynomial as the device applies it (test_gpu_parity: 5e-6 of the oracle's)
        ref = {}
        numpy_pcg(A, M, b, np.zeros(n), 0.0, 0, iters=max(got),
                  on_iterate=lambda k, x: ref.__setitem__(k, x.copy()) if k in got else None)
        out["drift"] = {k: relerr(got[k], ref[k]) for k in got}
        return out
    finally:
        gpu.close()


def bound(pre):
    return ITERATE_BOUND_F32 if pre == "cheb32" else ITERATE_BOUND


def check(out, pre):
    for k, d in out["drift"].items():
        assert d <= bound(pre), (k, d, bound(pre))


# ---- 1. single domain, default forms ------------------------------------------------------------------------------------------------
SINGLE = [(scene, pre) for scene in ("cavity32", "coil32", "spheres32", "blob6") for pre in PRECONDS if (scene, pre) not in ITERATE_DROPPED]


@pytest.mark.parametrize("scene,pre", SINGLE)
def test_iterates_match_the_reference(scene, pre):
    """x_25 and x_50 of the default step forms against the fp64 reference.  Measured max |dx| / max |x| on an MI355X (x_25 / x_50):
      cavity32  identity 5.1e-15 / 1.3e-14, Jacobi 7.5e-15 / 2.5e-14, Chebyshev-1 4.0e-15 / 1.2e-14, -2 9.7e-15 / 1.3e-14, -4 5.4e-15 / 5.5e-15,
                -10 6.9e-15, fp32 1.0e-9 / 2.7e-11
      coil32    identity 4.2e-15 / 1.1e-14, Jacobi 4.2e-15 / 6.0e-15, Chebyshev-1 6.2e-15 / 7.7e-15, -2 2.9e-15 / 2.9e-15, -4 8.9e-16 / 8.9e-16,
                -10 1.0e-15, fp32 2.3e-10 / 2.4e-10
      spheres32 identity 1.8e-15 / 4.5e-15, Jacobi 5.1e-15 / 4.1e-15, Chebyshev-1 4.1e-15 / 5.8e-15, -2 8.4e-14 / 4.5e-14, -4 5.2e-14 / 3.8e-14,
                -10 6.5e-14 / 1.3e-13, fp32 1.4e-8 / 4.1e-9
      blob6     identity 1.6e-15 / 5.6e-15, Jacobi 1.6e-15 / 2.7e-15, Chebyshev-1 9.2e-16 / 3.2e-15, -2 8.0e-16 / 8.0e-16, -4 1.0e-15,
                fp32 1.3e-11 / 2.6e-14
    The fp32 polynomial's bound cannot see a 1e-6 error of beta (it moves x by 8e-11 to 1.4e-7): a known gap, its self-check is the zeroed
    row only."""
    check(run_case(scene, pre), pre)


# ---- 2. forced forms, one child process per switch set --------------------------------------------------------------------------------
_CHILD = (
    "import test_gpu_iterates as t\n"
    "out = []\n"
    "for case in json.loads(sys.argv[1]):\n"
    "    r = t.run_case(case[0], case[1], ops=True)\n"
    "    r['case'] = case\n"
    "    out.append(r)\n"
    "print('RESULT ' + json.dumps(out))\n"
)


def run_child(env, cases, timeout=900):
    return children.run_python(_CHILD, json.dumps(cases), limit=timeout, env=env).result()


_PAIR = [["coil32", "jacobi"], ["spheres32", "cheb4"]]
FORCED = {
    "fused_r": ({"PS_FUSED_R": "1"}, [["cavity32", q] for q in PRECONDS] + [["coil32", "jacobi"], ["spheres32", "cheb32"]]),
    "nt_level2": ({"PS_NT_LEVEL": "2"}, _PAIR),
    "one_unit": ({"PS_S_DUAL": "0", "PS_ST_DUAL": "0"}, _PAIR + [["blob6", "identity"]]),
    "no_ell": ({"PS_NO_ELL": "1"}, _PAIR),
    "one_shot": ({"PS_PIPE_GRID": "0"}, _PAIR),
    "fp64_values": ({"PS_FORCE_FP64_VALUES": "1"}, _PAIR),
    "tile_split_valu": ({"PS_TILE_SPLIT": "1", "PS_TILE_VALU": "1"}, _PAIR),
    # walks: grids far below the chunk count (multiples of 8: the XCD walk and the fp32 polynomial stay on).  The two-unit kernels deal runs
    # of 32 pairs to the XCDs whatever PS_XCD says; the one-unit kernels' runs follow PS_XCD (1: one chunk, 3: rounded down to 2) and
    # PS_WG_RUN (log2 of the consecutive chunks a workgroup takes)
    "walk_grid": ({"PS_PIPE_GRID": "64", "PS_PIPE_GRID_ST": "40", "PS_XCD": "1"},
                  [["spheres48", "jacobi"], ["spheres48", "cheb4"], ["cavity48", "cheb32"]]),
    "walk_grid_fused": ({"PS_PIPE_GRID": "64", "PS_PIPE_GRID_ST": "24", "PS_XCD": "1", "PS_FUSED_R": "1"},
                        [["spheres48", "jacobi"], ["spheres48", "cheb4"], ["cavity48", "cheb32"]]),
    "walk_xcd3_run0": ({"PS_PIPE_GRID": "64", "PS_XCD": "3", "PS_WG_RUN": "0", "PS_S_DUAL": "0", "PS_ST_DUAL": "0"},
                       [["coil48", "jacobi"], ["spheres48", "identity"]]),
    "walk_run2": ({"PS_PIPE_GRID": "48", "PS_XCD": "1", "PS_WG_RUN": "2", "PS_S_DUAL": "0", "PS_ST_DUAL": "0", "PS_FUSED_R": "1"},
                  [["cavity48", "jacobi"], ["spheres48", "identity"]]),
}
WALK_SETS = {"walk_grid", "walk_grid_fused", "walk_xcd3_run0", "walk_run2"}


def walk_records(walk):
    return [w for w in walk if w[0] == 1]


@pytest.mark.parametrize("name", list(FORCED))
def test_forced_forms_match_the_reference(name):
    """each switch set in its own process (the switches are read once per process): x_25 / x_50 against the reference, apply(x) against the
    oracle to 1e-12 of max |y|, precondition(r) to 1e-10 (5e-6 for the fp32 polynomial).

    launchWalk counts the steps in which a workgroup gets a chunk.  Under the walk-forcing sets every workgroup of every persistent launch
    gets at least two, some workgroups get more than others (a partial last run), and where the two-unit kernels walk pairs some launch has
    an odd chunk count (a half-empty last pair: spheres48's St, 1073 chunks).  Measured on an MI355X (least / most steps): walk_grid
    spheres48 S 4 / 8, St 26 / 28 and 12 / 18 (Chebyshev term), cavity48 S 8 / 12, St 52 / 54 and 25 / 32; walk_grid_fused St 21 / 30 and
    42 / 54; walk_xcd3_run0 coil48 4 / 5 and 8 / 9, spheres48 9 / 10 and 16 / 17; walk_run2 cavity48 24 / 28 and 44 / 44, spheres48
    12 / 16 and 20 / 24.

    Measured drift (x_25, x_50), fp64 steps: fused_r cavity32 every preconditioner 5.1e-15 .. 3.2e-14, coil32 Jacobi 5.6e-15 / 6.9e-15;
    nt_level2, one_unit, no_ell, one_shot, fp64_values: coil32 Jacobi 4.2e-15 .. 7.2e-15, spheres32 Chebyshev-4 2.8e-14 .. 5.3e-14, blob6
    identity 1.6e-15 / 5.6e-15; tile_split_valu coil32 1.4e-14 / 1.8e-14; the walk sets 1.5e-15 .. 5.1e-14.  fp32 polynomial: fused_r
    cavity32 1.3e-9 / 2.1e-11, spheres32 9.5e-9 / 4.0e-9; walk sets cavity48 5.4e-9 .. 7.6e-9 / 3.3e-10 .. 5.3e-10."""
    env, cases = FORCED[name]
    res = run_child(env, cases)
    for r in res:
        pre = r["case"][1]
        check(r, pre)
        assert r["apply"] <= 1e-12, r
        assert r["precondition"] <= (5e-6 if pre == "cheb32" else 1e-10), r
        if env.get("PS_FUSED_R") == "1":
            assert r["fused"] == 1, r
    if name in WALK_SETS:
        ws = [w for r in res for w in walk_records(r["walk"]) if w[1] != 0]     # (kernel 0: the one-shot CSR launch of a mode without a walk)
        assert ws and all(w[6] >= 2 for w in ws), ws                        # every workgroup of every persistent launch got >= 2 chunks
        assert any(w[6] != w[7] for w in ws), ws                             # a partial last run
        if any(w[5] for w in ws):
            assert any(w[5] and w[2] % 2 == 1 for w in ws), ws               # a half-empty last pair


def all_cases():
    """every (scene, preconditioner) whose iterates a test here compares: the tolerance self-checks (test_iterate_tolerances_cpu.py) run on them"""
    return sorted(set(SINGLE) | {tuple(c) for _, cases in FORCED.values() for c in cases})

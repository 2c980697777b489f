"""The numpy restatement of the collider loads (collider_loads_ref.py) checked without a GPU: hand-worked single-entry cases, the mutants
the GPU test's bound must tell from the rule, and the adjointness that fixes sign and scale — the x-momentum the recovery takes from the
liquid, dx^3 sum (C x) over the rows of an axis, is the force on the solids along that axis.

Weights, labels and x come from the oracle's CPU setup and fp64 solve.  The adjointness needs every face with wF wL > 0 next to a DOF to
have a row of C (else the unmasked difference wF[hi] - wF[lo] counts a face the system does not hold): sliding_block and moving_floor at
n = 32 with doReducedRegions = 0 satisfy it, blob does not (344 faces inside its moving sphere lack a row) and is asserted not to."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import collider_loads_cases as cases  # noqa: E402
import collider_loads_ref as ref  # noqa: E402
import recovery_ref  # noqa: E402

from oracle import ps_oracle  # noqa: E402
from polystokes_amd import _abi as abi  # noqa: E402
from polystokes_amd import scenes  # noqa: E402

_runs = {}
oracle_solution = cases.oracle_solution


def oracle_run(name, reduced=True):
    """(scene, oracle, x, inputs of the restatement) of a scene; computed once, shared, never modified"""
    if (name, reduced) not in _runs:
        mk = {"moving32": lambda: scenes.moving_floor(32)}.get(name) or cases.SCENES[name]
        sc, p = mk()
        p.preconditioner = abi.PRE_DIAGONAL
        if not reduced:
            p.doReducedRegions = 0
        o = ps_oracle.Oracle()
        assert o.run(sc, p) == abi.SUCCESS
        x = o.array("solutionVector")
        _runs[(name, reduced)] = (sc, o, x, ref.inputs(o, sc, oracle_solution(o, x)))
    return _runs[(name, reduced)]


# ---- 1. hand-worked cases -------------------------------------------------------------------------------------------------------------------
def hand_inputs(n=(4, 5, 6), dx=0.5, orig=(1.0, 2.0, 3.0)):
    """wF_x = i / 8, wF_y = j / 8, wF_z = k / 8 (every difference along the own axis 1 / 8, none across); wL = 1 / 2 everywhere"""
    nx, ny, nz = n
    sh = abi.grid_shapes(nx, ny, nz)
    wF = []
    for a, name in enumerate(("faceX", "faceY", "faceZ")):
        idx = np.indices(sh[name])[2 - a]
        wF.append((idx / 8.0).astype(np.float32))
    return {"n": n, "dx": dx, "orig": orig, "wF": wF, "wC": np.ones(sh["center"], np.float32),
            "wL": {g: np.full(sh[g], 0.5, np.float32) for g in ("center",) + ref.EDGE_GRIDS},
            "sol": {k: np.zeros(sh[g], np.float32) for k, g in abi.SOLUTION_FIELDS}}


def test_single_pressure_entry_by_hand():
    inp = hand_inputs()
    inp["sol"]["pressure"][3, 2, 1] = 2.0                       # cell i = 1, j = 2, k = 3
    F, T, n, A, B = ref.loads(inp, 1)
    f = -0.25 * 0.5 * 2.0 * 0.125                               # -dx^2 wL P (1 / 8) on every axis
    arm = np.array([1.5, 2.5, 3.5]) * 0.5                       # the cell centre from the pivot orig
    assert list(n) == [3, 0]
    assert np.array_equal(F[0], [f, f, f]) and np.array_equal(A[0], [-f, -f, -f])
    assert np.array_equal(T[0], np.cross(arm, [f, f, f]))
    assert np.array_equal(B[0], [(arm[1] + arm[2]) * -f, (arm[0] + arm[2]) * -f, (arm[0] + arm[1]) * -f])


def test_single_normal_stress_entry_by_hand():
    inp = hand_inputs()
    inp["sol"]["tyy"][0, 4, 3] = -3.0                           # cell i = 3, j = 4, k = 0: the last cell along x and y
    piv = [[0.25, 0.5, 4.0]]
    F, T, n, A, B = ref.loads(inp, 1, pivots=piv)
    f = 0.25 * 0.5 * -3.0 * 0.125                               # +dx^2 wL Tyy (1 / 8), on y alone
    arm = np.array([1.0 + 3.5 * 0.5, 2.0 + 4.5 * 0.5, 3.0 + 0.5 * 0.5]) - piv[0]
    assert list(n) == [1, 0]
    assert np.array_equal(F[0], [0.0, f, 0.0]) and np.array_equal(A[0], [0.0, -f, 0.0])
    assert np.array_equal(T[0], [-(arm[2] * f), 0.0, arm[0] * f])
    assert np.array_equal(B[0], [abs(arm[2] * f), 0.0, abs(arm[0] * f)])


def test_single_shear_entry_by_hand():
    """T_xy on the XY edge (i, j, k) = (2, 3, 1): the x term differences wF_x along y, the y term wF_y along x; with the ramps above both
    are 0, so the x-face weights get a step in y and the y-face weights a step in x"""
    inp = hand_inputs()
    inp["wF"][0][:, 3:, :] += np.float32(0.25)                  # wF_x[e] - wF_x[e - e_y] = 1 / 4 at j = 3
    inp["wF"][1][:, :, 2:] -= np.float32(0.5)                   # wF_y[e] - wF_y[e - e_x] = -1 / 2 at i = 2
    inp["sol"]["txy"][1, 3, 2] = 4.0
    F, T, n, A, B = ref.loads(inp, 1)
    fx, fy = 0.25 * 0.5 * 4.0 * 0.25, 0.25 * 0.5 * 4.0 * -0.5
    arm = np.array([2 * 0.5, 3 * 0.5, 1.5 * 0.5])               # x and y on grid lines, z at the half cell
    assert list(n) == [2, 0]
    assert np.array_equal(F[0], [fx, fy, 0.0]) and np.array_equal(A[0], [fx, -fy, 0.0])
    assert np.array_equal(T[0], np.cross(arm, [fx, fy, 0.0]))
    # a border edge: the lower face of the x term lies outside the x-face grid, the y term stays
    inp["sol"]["txy"][:] = 0
    inp["sol"]["txy"][1, 0, 2] = 4.0
    F, T, n, A, B = ref.loads(inp, 1)
    assert list(n) == [1, 0] and F[0, 0] == 0.0 and F[0, 1] == fy


def test_attribution_by_hand():
    """ids: a cell term takes its cell's id; an edge term the id of the in-grid neighbour with the smallest centre fluid weight, ties to the
    lowest index; ids outside the count are dropped and counted"""
    inp = hand_inputs()
    inp["wF"][0][:, 3:, :] += np.float32(0.25)
    inp["sol"]["txy"][1, 3, 2] = 4.0                            # cells around: (i, j) in {1, 2} x {2, 3}, k = 1
    inp["sol"]["pressure"][0, 0, 0] = 1.0
    ids = np.zeros((6, 5, 4), np.int32)
    ids[1, 2, 1], ids[1, 2, 2], ids[1, 3, 1], ids[1, 3, 2] = 1, 2, 3, 4
    ids[0, 0, 0] = 9
    F, T, n, A, B = ref.loads(inp, 5, ids=ids)
    assert list(n) == [0, 1, 0, 0, 0, 3]                        # a four-way tie: the lowest cell (id 1); the pressure cell's three terms dropped
    inp["wC"][1, 3, 1] = 0.5
    assert list(ref.loads(inp, 5, ids=ids)[2]) == [0, 0, 0, 1, 0, 3]
    inp["wC"][1, 2, 2] = 0.5                                    # a tie of two: the lower index
    assert list(ref.loads(inp, 5, ids=ids)[2]) == [0, 0, 1, 0, 0, 3]
    ids[1, 2, 2] = -1
    assert list(ref.loads(inp, 5, ids=ids)[2]) == [0, 0, 0, 0, 0, 4]


# ---- 2. mutants -----------------------------------------------------------------------------------------------------------------------------
MUTANT_CASES = [("blob", "none"), ("spheres32", "spheres"), ("spheres32", "mod3"), ("sliding32", "none")]


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_mutant_leaves_the_bound_on_some_case(mutant):
    caught = []
    for name, kind in MUTANT_CASES:
        sc, o, x, inp = oracle_run(name)
        count = 8 if kind == "spheres" else (3 if kind == "mod3" else 1)
        ids = cases.ids_field(sc, kind)
        piv = cases.pivots_for(sc, count, "spheres" if kind == "spheres" else None)
        want = ref.loads(inp, count, ids, piv)
        assert int(want[2][:-1].sum()) > 100, (name, kind, want[2])                   # the case has terms to be wrong about
        assert ref.outside(want, want) == []
        if ref.outside(ref.loads(inp, count, ids, piv, mutant=mutant), want):
            caught.append((name, kind))
    assert caught, mutant


def test_the_spheres_case_drops_terms_and_fills_eight_colliders():
    sc, o, x, inp = oracle_run("spheres32")
    n = ref.loads(inp, 8, cases.ids_field(sc, "spheres"), cases.pivots_for(sc, 8, "spheres"))[2]
    assert n[8] > 0 and np.all(n[:8] > 0), n


# ---- 3. adjointness -------------------------------------------------------------------------------------------------------------------------
def faces_without_a_row(sc, o, b, inp):
    """faces with wF wL > 0 next to a DOF that have no row of C"""
    sh = abi.grid_shapes(sc.nx, sc.ny, sc.nz)
    rows = [b.face_rows[a].reshape(sh["face" + "XYZ"[a]]) for a in range(3)]
    miss = 0
    idx = np.nonzero(o.array("centerActiveIndices").reshape(sh["center"]) >= 0)
    wl = inp["wL"]["center"][idx]
    for a in range(3):
        for q in (0, 1):
            f = ref._shift(idx, a, q)
            miss += int(((inp["wF"][a][f] * wl > 0) & (rows[a][f] < 0)).sum())
    for ea, grid in enumerate(ref.EDGE_GRIDS):
        idx = np.nonzero(o.array(grid + "ActiveIndices").reshape(sh[grid]) >= 0)
        wl = inp["wL"][grid][idx]
        p0, p1 = (1 if ea == 0 else 0), (1 if ea == 2 else 2)
        for a, other in ((p0, p1), (p1, p0)):
            for q in (0, -1):
                f = ref._shift(idx, other, q)
                ok = ref._inside(f, inp["wF"][a].shape)
                ff = tuple(t[ok] for t in f)
                miss += int(((inp["wF"][a][ff] * wl[ok] > 0) & (rows[a][ff] < 0)).sum())
    return miss, rows


@pytest.mark.parametrize("name", ["sliding32", "moving32"])
def test_force_is_the_adjoint_of_the_recovery(name):
    sc, o, x, inp = oracle_run(name, reduced=False)
    b = recovery_ref.from_oracle(o, sc)
    miss, rows = faces_without_a_row(sc, o, b, inp)
    assert miss == 0                                                            # the precondition
    F, T, n, A, B = ref.loads(inp, 1)
    assert n[0] > 1000 and n[1] == 0
    Cx, aCx = b.C @ x, abs(b.C) @ np.abs(x)
    big = 0.0
    for a in range(3):
        r = rows[a][rows[a] >= 0]
        lhs = sc.dx ** 3 * Cx[r].sum()
        bound = 2.0 ** -24 * sc.dx ** 3 * aCx[r].sum() + (n[0] + 8) * ref.U64 * A[:, a].sum()
        print(name, "axis", a, "dx^3 sum(C x)", lhs, "F", F[0, a], "difference", abs(lhs - F[0, a]), "bound", bound)
        assert abs(lhs - F[0, a]) <= bound, (a, lhs, F[0, a], bound)
        big = max(big, abs(F[0, a]) / bound)
    assert big > 1e3                                                            # the equality is not vacuous: some force stands far above the bound


def test_blob_does_not_meet_the_precondition():
    sc, o, x, inp = oracle_run("blob", reduced=False)
    miss, _ = faces_without_a_row(sc, o, recovery_ref.from_oracle(o, sc), inp)
    assert miss > 0

"""numpy restatement of the free-surface fields (include/polystokes.h, ps_upload_surface_fields): the ghost pressure q_c = s_c kappa_c + P_c
per cell, the sum t_f = sum_c sign wF ghost_c invDx q_c per face in the library's order of operations, and the impulse -dt t_f in the active
rhs, in the tiles' rhs through C_f^T, and in b.  The grid functions take plain arrays (the CPU tests feed them synthetic grids); the
solver functions read the exported arrays.  The helpers are those of tests/test_gpu_surface_tension.py with q_c in the place of kappa_c."""
import numpy as np

from polystokes_amd import _abi as abi
from helpers import basis_rows


def active_label(l):
    return (l == abi.ACTIVEFLUID) | (l == abi.BOUNDARY)


def ghost_pressure(kappa, sigma_field=None, sigma=0.0, pressure_field=None):
    """q_c in fp64.  kappa: the fp32 "surfaceCurvature", or None when neither a sigma field nor a scalar sigma > 0 asks for it (the term is
    then absent).  sigma_field / pressure_field: fp32 cell fields or None (the scalar `sigma` / 0)."""
    P = 0.0 if pressure_field is None else np.asarray(pressure_field, np.float32).astype(np.float64)
    if kappa is None:
        return np.array(P, np.float64)
    s = float(sigma) if sigma_field is None else np.asarray(sigma_field, np.float32).astype(np.float64)
    return s * np.asarray(kappa, np.float32).astype(np.float64) + P


def ghost_fraction(lab, lw):
    """1 - liquidW_c for a cell with an active label or REDUCED, 1 for any other cell"""
    return np.where(active_label(lab) | (lab == abi.REDUCED), 1.0 - np.asarray(lw, np.float64), 1.0)


def face_sums(frac, wf, val, dx):
    """per face grid (X, Y, Z): t = 0; t += -wF frac invDx val of the lower cell, then t += +wF frac invDx val of the upper cell, each
    product left to right, cells outside the grid and cells with frac == 0 skipped, 0 where wF == 0.  frac / val: (nz, ny, nx) cell grids;
    wf: the three face fluid-weight grids; dx: the cell size."""
    inv = 1.0 / float(dx)
    frac, val = np.asarray(frac, np.float64), np.asarray(val, np.float64)
    out = []
    for a in range(3):
        ax = 2 - a
        w = np.asarray(wf[a], np.float64)
        none = np.zeros_like(np.take(frac, [0], axis=ax))
        f_lo, v_lo = np.concatenate([none, frac], axis=ax), np.concatenate([none, val], axis=ax)      # cell f - 1 (none below face 0)
        f_hi, v_hi = np.concatenate([frac, none], axis=ax), np.concatenate([val, none], axis=ax)      # cell f (none above the last face)
        lower = np.where(f_lo != 0, (((-1.0 * w) * f_lo) * inv) * v_lo, 0.0)
        upper = np.where(f_hi != 0, (((1.0 * w) * f_hi) * inv) * v_hi, 0.0)
        out.append(np.where(w != 0, (0.0 + lower) + upper, 0.0))
    return out


def ghost_sums(lab, lw, wf, val, dx):
    """t_f = sum_c g(f,c) val_c: face_sums with the ghost fraction of every cell"""
    return face_sums(ghost_fraction(lab, lw), wf, val, dx)


def liquid_gradient(lab, lw, wf, val, dx):
    """sum_c sign wF liquid_c invDx val_c with the stencil's liquid-side fraction: liquidW_c for a cell with a pressure DOF (active label
    or REDUCED), 0 for any other cell"""
    return face_sums(np.where(active_label(lab) | (lab == abi.REDUCED), np.asarray(lw, np.float64), 0.0), wf, val, dx)


def solver_ghost_sums(solver, sc, q):
    """ghost_sums on the exported labels and weights of the last setup"""
    sh = abi.grid_shapes(sc.nx, sc.ny, sc.nz)
    lab = solver.array("centerLabels").reshape(sh["center"])
    lw = solver.array("centerLiquidWeights").reshape(sh["center"])
    wf = [solver.array("face" + "XYZ"[a] + "FluidWeights").reshape(sh["face" + "XYZ"[a]]) for a in range(3)]
    return ghost_sums(lab, lw, wf, np.asarray(q).reshape(sh["center"]), sc.dx)


def per_row(solver, per_face):
    """a per-face quantity in the order of the active rows (reference numbering: the X faces, then Y, then Z; face*ActiveIndices number
    each axis from 0, so a face's row is its index plus the active faces of the axes before it)"""
    vals = np.full(solver.nA, np.nan)
    off = 0
    for a in range(3):
        act = solver.array("face" + "XYZ"[a] + "ActiveIndices")
        m = act >= 0
        assert act[m].min(initial=0) == 0 and act[m].max(initial=-1) == int(m.sum()) - 1
        vals[act[m] + off] = per_face[a].ravel()[m]
        off += int(m.sum())
    assert off == solver.nA and not np.isnan(vals).any()
    return vals


def reduced_impulse(solver, sc, sums, scale):
    """sum over each region's reduced faces of C_f^T (-scale t_f), and the number of faces with a non-zero impulse"""
    sh = abi.grid_shapes(sc.nx, sc.ny, sc.nz)
    com = solver.array("reducedRegionCOM").reshape(-1, 3)
    R = solver.nRegions
    out = np.zeros((R, 26))
    hits = 0
    for a in range(3):
        n = "face" + "XYZ"[a]
        lab = solver.array(n + "Labels").reshape(sh[n])
        red = solver.array(n + "ReducedIndices").reshape(sh[n])
        k, j, i = np.nonzero((lab == abi.REDUCED) & (red >= 0) & (sums[a] != 0))
        hits += len(i)
        pos = np.stack([i, j, k], axis=1).astype(np.float64)
        pos[:, a] -= 0.5
        r = red[k, j, i]
        C = basis_rows(pos * sc.dx - com[r], np.full(len(r), a))
        np.add.at(out, r, C * (-scale * sums[a][k, j, i])[:, None])
    return out, hits


def delta_b(solver, sc, d_rhs_a, d_rhs_r):
    """b = -S^T t0 + [rhs_p; rhs_tau], t0 = McInv rhs_a on the active rows and C_f (invDt BInv_r rhs_r) on the reduced rows
    (ps_solve.hip: assembleSystemPressureStressFactored): the change of b for a change of the two rhs vectors"""
    S, _ = solver.S_matrices()
    nA = solver.nA
    t0 = np.zeros(S.shape[0])
    t0[:nA] = solver.array("McInv") * d_rhs_a
    faces = solver.array("reducedRowFace").astype(np.int64)
    if len(faces):
        R = solver.nRegions
        binv = solver.array("Inv_Mr_plus_2JDtuDJ").reshape(R, 26, 26)
        w = np.einsum("rij,rj->ri", binv, d_rhs_r.reshape(R, 26)) / sc.dt
        reg = solver.array("reducedRowRegion")
        com = solver.array("reducedRegionCOM").reshape(-1, 3)
        i, j, k, ax = faces & 1023, (faces >> 10) & 1023, (faces >> 20) & 1023, faces >> 30
        pos = np.stack([i, j, k], axis=1).astype(np.float64)
        pos[np.arange(len(ax)), ax] -= 0.5
        C = basis_rows(pos * sc.dx - com[reg], ax)
        t0[nA:nA + len(faces)] = np.einsum("ki,ki->k", C, w[reg])
    return -(S.T @ t0)


def expected_changes(solver, sc, q):
    """(change of activeRHSVector, change of reducedRHSVector as (R, 26), reduced faces with an impulse, change of b) of a setup whose ghost
    pressure is q against the same setup without any surface term"""
    sums = solver_ghost_sums(solver, sc, q)
    d_a = -sc.dt * per_row(solver, sums)
    d_r, hits = reduced_impulse(solver, sc, sums, sc.dt)
    return d_a, d_r, hits, delta_b(solver, sc, d_a, d_r.ravel())

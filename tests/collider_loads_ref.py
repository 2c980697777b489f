"""Collider loads (ps_set_collider_loads) restated in numpy, fp64: include/polystokes.h states every term, this module forms the same
terms with the same products in the same order, so a term here has the bits of the device's.  The sums are exact (math.fsum, rounded
once): a device sum in any order lies within (terms + 8) 2^-53 A of them — terms - 1 additions of at most 2^-53 of the running sum, which
A bounds, and the rounding of the reference itself.

Arrays are (z, y, x) numpy arrays, x fastest, as everywhere in the tests.  inputs(): the dict loads() reads, from a Solver or an Oracle."""
import math

import numpy as np

from polystokes_amd import _abi as abi

U64 = 2.0 ** -53
EDGE_GRIDS = ("edgeYZ", "edgeXZ", "edgeXY")           # edge axis 0, 1, 2: the in-plane axes are the other two
EDGE_SOLUTION = ("tyz", "txz", "txy")
MUTANTS = ("shear_sign", "edge_plus", "no_wl", "corner_arm", "lowest_cell_id")


def inputs(src, scene, sol):
    """src: a Solver or an Oracle after a step (its weight arrays); sol: the seven fp32 grids keyed like Solver.solution_fields()"""
    sh = abi.grid_shapes(scene.nx, scene.ny, scene.nz)
    grid = lambda name, kind: np.asarray(src.array(name + kind + "Weights"), np.float32).reshape(sh[name])
    return {"n": (scene.nx, scene.ny, scene.nz), "dx": float(scene.dx), "orig": tuple(float(v) for v in getattr(scene, "orig", (0.0, 0.0, 0.0))),
            "wF": [grid("face" + a, "Fluid") for a in "XYZ"], "wC": grid("center", "Fluid"),
            "wL": {name: grid(name, "Liquid") for name in ("center",) + EDGE_GRIDS},
            "sol": {k: np.asarray(sol[k], np.float32).reshape(sh[g]) for k, g in abi.SOLUTION_FIELDS}}


def _shift(idx, axis, q):
    """the (k, j, i) index arrays moved q steps along axis (0 = x: the last array dimension)"""
    out = list(idx)
    out[2 - axis] = out[2 - axis] + q
    return tuple(out)


def _inside(idx, shape):
    ok = np.ones(idx[0].shape, bool)
    for v, n in zip(idx, shape):
        ok &= (v >= 0) & (v < n)
    return ok


def _terms(inp, ids, mutant):
    """every term as (axis, f, position (n, 3) in x y z, collider id)"""
    dx, orig = inp["dx"], np.asarray(inp["orig"], np.float64)
    dx2 = dx * dx
    out = []
    sol, wF = inp["sol"], inp["wF"]

    def position(idx, half):
        """orig + (index + 0.5) dx on the axes of `half`, orig + index dx on the others"""
        cols = []
        for a in range(3):
            v = idx[2 - a].astype(np.float64)
            cols.append(orig[a] + ((v + 0.5) if a in half else v) * dx)
        return np.stack(cols, axis=1)

    # cells: pressure and normal stress on each axis
    P, Taa = sol["pressure"], [sol["txx"], sol["tyy"], sol["tzz"]]
    idx = np.nonzero((P != 0) | (Taa[0] != 0) | (Taa[1] != 0) | (Taa[2] != 0))
    wl = inp["wL"]["center"][idx].astype(np.float64)
    if mutant == "no_wl":
        wl = np.ones_like(wl)
    pos = position(idx, () if mutant == "corner_arm" else (0, 1, 2))
    cid = np.zeros(len(idx[0]), np.int64) if ids is None else ids[idx].astype(np.int64)
    for a in range(3):
        d = wF[a][_shift(idx, a, 1)].astype(np.float64) - wF[a][idx].astype(np.float64)
        for val, sign in ((P, -1.0), (Taa[a], 1.0)):
            v = val[idx].astype(np.float64)
            m = (d != 0) & (v != 0)
            out.append((a, ((sign * dx2 * wl[m]) * v[m]) * d[m], pos[m], cid[m]))
    # edges: shear on each in-plane axis
    nz, ny, nx = inp["wC"].shape
    for ea in range(3):
        tau = sol[EDGE_SOLUTION[ea]]
        idx = np.nonzero(tau != 0)
        v = tau[idx].astype(np.float64)
        wl = inp["wL"][EDGE_GRIDS[ea]][idx].astype(np.float64)
        if mutant == "no_wl":
            wl = np.ones_like(wl)
        pos = position(idx, () if mutant == "corner_arm" else (ea,))
        p0, p1 = (1 if ea == 0 else 0), (1 if ea == 2 else 2)
        if ids is None:
            eid = np.zeros(len(v), np.int64)
        else:
            eid = np.full(len(v), -1, np.int64)
            best = np.full(len(v), np.inf)
            have = np.zeros(len(v), bool)
            for q in range(4):                       # rising x-fastest cell index: the strict comparison keeps the lowest index of a tie
                c = _shift(_shift(idx, p1, (q >> 1) - 1), p0, (q & 1) - 1)
                ok = _inside(c, (nz, ny, nx))
                cc = tuple(np.where(ok, t, 0) for t in c)
                w = inp["wC"][cc].astype(np.float64)
                take = ok & (~have | (w < best))
                if mutant == "lowest_cell_id":
                    take = ok & ~have
                best = np.where(take, w, best)
                eid = np.where(take, ids[cc].astype(np.int64), eid)
                have |= ok
        for a, b in ((p0, p1), (p1, p0)):
            lo = _shift(idx, b, 1 if mutant == "edge_plus" else -1)
            ok = _inside(idx, wF[a].shape) & _inside(lo, wF[a].shape)
            hi_i = tuple(t[ok] for t in idx)
            lo_i = tuple(t[ok] for t in lo)
            d = wF[a][hi_i].astype(np.float64) - wF[a][lo_i].astype(np.float64)
            m = d != 0
            sign = -1.0 if mutant == "shear_sign" else 1.0
            out.append((a, ((sign * dx2 * wl[ok][m]) * v[ok][m]) * d[m], pos[ok][m], eid[ok][m]))
    return out


def loads(inp, count, ids=None, pivots=None, mutant=None):
    """F (count, 3), T (count, 3), counts (count + 1: the last entry is the dropped terms), A (count, 3), B (count, 3)"""
    assert mutant is None or mutant in MUTANTS, mutant
    piv = np.tile(np.asarray(inp["orig"], np.float64), (count, 1)) if pivots is None else np.asarray(pivots, np.float64).reshape(count, 3)
    if ids is not None:
        ids = np.asarray(ids).reshape(inp["wC"].shape)
    F, T, A, B = (np.zeros((count, 3)) for _ in range(4))
    counts = np.zeros(count + 1, np.int32)
    addF = [[[] for _ in range(3)] for _ in range(count)]
    addT = [[[] for _ in range(3)] for _ in range(count)]
    for a, f, pos, cid in _terms(inp, ids, mutant):
        good = (cid >= 0) & (cid < count)
        counts[count] += int((~good).sum())
        a1, a2 = (a + 1) % 3, (a + 2) % 3
        for k in np.unique(cid[good]):
            m = cid == k
            arm = pos[m] - piv[k]
            fk = f[m]
            counts[k] += len(fk)
            addF[k][a].append(fk)
            addT[k][a1].append(arm[:, a2] * fk)
            addT[k][a2].append(-(arm[:, a1] * fk))
    for k in range(count):
        for a in range(3):
            f = np.concatenate(addF[k][a]) if addF[k][a] else np.zeros(0)
            t = np.concatenate(addT[k][a]) if addT[k][a] else np.zeros(0)
            F[k, a], A[k, a] = math.fsum(f), math.fsum(np.abs(f))
            T[k, a], B[k, a] = math.fsum(t), math.fsum(np.abs(t))
    return F, T, counts, A, B


def bound(terms, scale):
    """|sum - reference| <= (terms + 8) 2^-53 scale, per collider (terms: (count,), scale: (count, 3))"""
    return (np.asarray(terms, np.float64)[:, None] + 8.0) * U64 * np.asarray(scale, np.float64)


def outside(got, want):
    """what of got = (F, T, counts, A, B) leaves the bound around want, as a list of strings (empty: inside)"""
    F, T, n, A, B = want
    gF, gT, gn, gA, gB = got
    bad = []
    if not np.array_equal(np.asarray(gn), n):
        bad.append("counts %s != %s" % (list(gn), list(n)))
    bF, bT = bound(n[:-1], A), bound(n[:-1], B)
    for name, g, w, b in (("F", gF, F, bF), ("T", gT, T, bT), ("A", gA, A, bF), ("B", gB, B, bT)):
        d = np.abs(np.asarray(g, np.float64) - w)
        if not np.all(d <= b):                                     # (a NaN is outside)
            k, a = np.unravel_index(int(np.argmax(np.where(d <= b, 0.0, np.where(np.isnan(d), np.inf, d)))), d.shape)
            bad.append("%s[%d][%d] = %r, reference %r, bound %.3e" % (name, k, a, float(np.asarray(g)[k, a]), float(w[k, a]), float(b[k, a])))
    return bad

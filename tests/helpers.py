import math

import numpy as np
import pytest
import scipy.sparse as sp

from polystokes_amd import _abi as abi
from polystokes_amd import scenes


def basis_rows(off, axis):
    """Vectorised C_a(x) (exec/HDK_PolyStokesSolver.cpp:2105-2149).  off: (n,3), axis: (n,) -> (n,26)."""
    off = np.asarray(off, np.float64)
    axis = np.asarray(axis)
    x, y, z = off[:, 0], off[:, 1], off[:, 2]
    n = len(x)
    C = np.zeros((n, 26))
    quad = np.stack([x, y, z, x * x, x * y, x * z, y * y, y * z, z * z], axis=1)
    m0, m1, m2 = axis == 0, axis == 1, axis == 2
    C[m0, 0] = 1
    C[np.ix_(m0, range(3, 12))] = quad[m0]
    C[m1, 1] = 1
    C[np.ix_(m1, range(12, 21))] = quad[m1]
    C[m2, 2] = 1
    C[m2, 3] = -z[m2]
    C[m2, 6] = -2 * x[m2] * z[m2]
    C[m2, 7] = -y[m2] * z[m2]
    C[m2, 8] = -0.5 * z[m2] * z[m2]
    C[m2, 13] = -z[m2]
    C[m2, 16] = -x[m2] * z[m2]
    C[m2, 18] = -2 * y[m2] * z[m2]
    C[m2, 19] = -0.5 * z[m2] * z[m2]
    C[m2, 21] = x[m2]
    C[m2, 22] = y[m2]
    C[m2, 23] = x[m2] * x[m2]
    C[m2, 24] = x[m2] * y[m2]
    C[m2, 25] = y[m2] * y[m2]
    return C


def materialise_blocks(solver):
    """G, Dt, JG, JDt (scipy CSR) from the device's factored storage S = [G Dt; Ghat Dhat] and the
    on-the-fly basis — what exportComponentMatrices() writes (Solver.cpp:557-560)."""
    S, _ = solver.S_matrices()
    nA, nP, R = solver.nA, solver.nP, solver.nRegions
    G, Dt = S[:nA, :nP].tocsr(), S[:nA, nP:].tocsr()
    packed = solver.array("reducedRowFace")
    reg = solver.array("reducedRowRegion")
    nRr = len(packed)
    if nRr == 0:
        JG = sp.csr_matrix((R * 26, nP))
        JDt = sp.csr_matrix((R * 26, S.shape[1] - nP))
        return G, Dt, JG, JDt
    i, j, k, a = packed & 1023, (packed >> 10) & 1023, (packed >> 20) & 1023, packed >> 30
    pos = np.stack([i, j, k], axis=1).astype(np.float64)
    pos[np.arange(nRr), a] -= 0.5
    com = solver.array("reducedRegionCOM").reshape(-1, 3)
    off = pos * solver.scene.dx - com[reg]
    Cm = basis_rows(off, a)
    rows = (reg[:, None] * 26 + np.arange(26)[None, :]).ravel()
    cols = np.repeat(np.arange(nRr), 26)
    J = sp.csr_matrix((Cm.ravel(), (rows, cols)), shape=(R * 26, nRr))
    Sr = S[nA:, :]
    JG = (J @ Sr[:, :nP]).tocsr()
    JDt = (J @ Sr[:, nP:]).tocsr()
    return G, Dt, JG, JDt


def per_row(solver, per_face):
    """a per-face quantity (three face grids) in the order of the active rows (McInv, Mc, activeRHSVector: reference numbering); solver: a
    Solver or an Oracle"""
    vals = np.full(solver.nA, np.nan)
    off = 0
    for a in range(3):
        act = solver.array("face" + "XYZ"[a] + "ActiveIndices")
        m = act >= 0
        base = off if act[m].min(initial=off) < off else 0      # axis-local or global numbering: both handled
        vals[act[m] + base] = np.asarray(per_face[a]).ravel()[m]
        off += int(m.sum())
    assert off == solver.nA and not np.isnan(vals).any()
    return vals


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.abs(a - b).max() if a.size else 0.0
    s = max(np.abs(b).max() if b.size else 0.0, 1e-300)
    return d / s


# ---- the system vector as grid fields (for comparisons between decompositions) -------------------------------------------
DOF_KINDS = ("p", "txx", "tyy", "tzz", "eYZ", "eXZ", "eXY")


def dof_field(solver, kind, x, dtype=np.float32):
    """One kind of DOF of a system vector x (reference numbering, Solver.h:586-606: pressures, then txx, tyy, tzz by cell, then the
    YZ / XZ / XY edge stresses) as a dense array over its sample grid, NaN where there is no DOF."""
    cidx = solver.array("centerActiveIndices")
    nP = int((cidx >= 0).sum())                    # (a slab rank's own count: its stats object holds the group's)
    if kind in ("p", "txx", "tyy", "tzz"):
        idx = cidx
        off = {"p": 0, "txx": nP, "tyy": 2 * nP, "tzz": 3 * nP}[kind]
    else:
        nE = [int((solver.array(s + "ActiveIndices") >= 0).sum()) for s in ("edgeYZ", "edgeXZ")]
        idx = solver.array({"eYZ": "edgeYZ", "eXZ": "edgeXZ", "eXY": "edgeXY"}[kind] + "ActiveIndices")
        off = 4 * nP + {"eYZ": 0, "eXZ": nE[0], "eXY": nE[0] + nE[1]}[kind]
    out = np.full(idx.shape, np.nan, dtype)
    m = idx >= 0
    out[m] = x[idx[m].astype(np.int64) + off]
    return out


def merge_dof_field(global_out, local, slab, kind):
    """Copy the DOFs a rank OWNS (cells and XY edges of its layers; YZ / XZ edges on its planes, the plane on a cut belonging to
    the rank above: DESIGN.md section 6) from its local field (x-fastest, local layers) into the global one."""
    nzl = slab.nz_local + (1 if kind in ("eYZ", "eXZ") else 0)
    loc = local.reshape(nzl, -1)
    glo = global_out.reshape(global_out.size // loc.shape[1], loc.shape[1])
    k0, k1 = slab.zLoOwned, slab.zHiOwned
    if kind in ("eYZ", "eXZ") and not slab.hasUpper:
        k1 += 1                                   # the top plane of the whole domain
    glo[slab.g0 + k0:slab.g0 + k1] = loc[k0:k1]


def merge_dof_field_brick(global_out, local, b, kind, global_n):
    """The same for a brick (partition.Brick): along every axis a kind lives in the cell layers or on the planes (plane-type axes per
    kind below), owned range [lo, hi) plus the last plane of the domain where there is no upper neighbour.  global_n = (nx, ny, nz)."""
    planes = {"p": (), "txx": (), "tyy": (), "tzz": (), "eYZ": (1, 2), "eXZ": (0, 2), "eXY": (0, 1)}[kind]
    lshape = tuple(b.n_local[a] + (1 if a in planes else 0) for a in (2, 1, 0))
    gshape = tuple(global_n[a] + (1 if a in planes else 0) for a in (2, 1, 0))
    loc, glo = local.reshape(lshape), global_out.reshape(gshape)
    sl_l, sl_g = [], []
    for a in (2, 1, 0):
        k0, k1 = b.lo[a], b.hi[a] + (1 if (a in planes and not b.hasUpper[a]) else 0)
        sl_l.append(slice(k0, k1)); sl_g.append(slice(b.origin[a] + k0, b.origin[a] + k1))
    glo[tuple(sl_g)] = loc[tuple(sl_l)]


def dof_numbering(solver):
    """(where, n) of a single domain: the DOF number at every sample of every kind, NaN where there is none.  solver: a Solver after its
    setup, or an Oracle after its run"""
    n = solver.nP + solver.nT
    where = {k: dof_field(solver, k, np.arange(n, dtype=np.float64), np.float64) for k in DOF_KINDS}
    assert sum(int((~np.isnan(w)).sum()) for w in where.values()) == n
    return where, n


def merged_x(where, n, grp, sc):
    """the owned DOFs of every rank's solutionVector as one x in the single domain's numbering (where: the DOF number at every sample).
    grp: a Group after set_scene, or anything with its `ranks` (each with .array(name)), `slabs` (the parts) and `dims`"""
    x = np.full(n, np.nan)
    for kind in DOF_KINDS:
        merged = np.full(where[kind].shape, np.nan)
        for r, part in enumerate(grp.slabs):
            loc = dof_field(grp.ranks[r], kind, grp.ranks[r].array("solutionVector"), np.float64)
            if grp.dims is None:
                merge_dof_field(merged, loc, part, kind)
            else:
                merge_dof_field_brick(merged, loc, part, kind, (sc.nx, sc.ny, sc.nz))
        assert np.array_equal(np.isnan(merged), np.isnan(where[kind])), kind            # the same DOFs exist
        m = ~np.isnan(merged)
        x[where[kind][m].astype(np.int64)] = merged[m]
    assert not np.isnan(x).any()
    return x


RANK_ARRAYS = ("solutionVector",) + tuple(s + "ActiveIndices" for s in ("center", "faceX", "faceY", "faceZ", "edgeYZ", "edgeXZ", "edgeXY"))


class SavedRanks:
    """what merged_x reads of a group, over arrays the ranks saved: saved[r] maps the names of RANK_ARRAYS to rank r's arrays (an npz does)"""

    class _Rank:
        def __init__(self, data):
            self.data = data

        def array(self, name):
            return self.data[name]

    def __init__(self, saved, parts, dims):
        self.ranks = [SavedRanks._Rank(d) for d in saved]
        self.slabs, self.dims = parts, (tuple(dims) if dims is not None else None)


def make_parts(sc, tile, world, dims):
    """the slabs (dims None) or bricks of every rank, as Group.set_scene cuts them"""
    from polystokes_amd import partition
    if dims is None:
        return [partition.make_slab(sc.nz, world, r, tile) for r in range(world)]
    return [partition.make_brick((sc.nx, sc.ny, sc.nz), dims, r, tile) for r in range(world)]


# ---- the random brick cases of scripts/fuzz_bricks.py (seed -> scene, parameters, decomposition) ---------------------------------
FUZZ_BRICK_DIMS = [(2, 2, 1), (2, 1, 2), (1, 2, 2), (2, 2, 2), (3, 1, 2), (1, 3, 2), (2, 2, 3)]


def fuzz_brick_case(seed, tol=1e-6):
    """One random blob scene with a free surface, its parameters and a brick decomposition, all drawn from RandomState(seed)."""
    from polystokes_amd import scenes
    rng = np.random.RandomState(seed)
    dims = FUZZ_BRICK_DIMS[int(rng.randint(len(FUZZ_BRICK_DIMS)))]
    tile = int(rng.choice([8, 16, 16]))
    n = [16 * int(rng.randint(d, d + 2)) if d > 1 else int(rng.randint(16, 40)) for d in dims]
    n = [max(v, 16 * d) for v, d in zip(n, dims)]
    sc, p = scenes.blob(n[0], n[1], n[2], seed=seed, tile=tile, pad=int(rng.choice([1, 2])), variable_viscosity=bool(rng.randint(2)))
    p.preconditioner = int(rng.choice([abi.PRE_IDENTITY, abi.PRE_DIAGONAL, abi.PRE_CHEBYSHEV]))
    p.activeLiquidBoundaryLayerSize = int(rng.choice([1, 2, 3])); p.activeSolidBoundaryLayerSize = int(rng.choice([0, 1, 2]))
    p.tolerance = float(tol)
    p.maxSolverIterations = 20000
    return sc, p, dims, n, tile


def rigid_rotation_scene(n=24, w=(0.3, -0.2, 0.5)):
    """the droplet scene with u = w x (x - centre) sampled on its faces; returns (scene, params, the three face arrays flattened)"""
    sc, p = scenes.droplet(n)
    dx = sc.dx
    w = np.array(w)
    c = np.array([0.5, 0.5, 0.5])
    ref = []
    for a in range(3):
        shp = [n, n, n]
        shp[a] += 1
        i, j, k = np.meshgrid(np.arange(shp[0]), np.arange(shp[1]), np.arange(shp[2]), indexing="ij")      # (x, y, z) index order
        pos = [(i + (0.0 if a == 0 else 0.5)) * dx - c[0], (j + (0.0 if a == 1 else 0.5)) * dx - c[1], (k + (0.0 if a == 2 else 0.5)) * dx - c[2]]
        u = np.cross(w, np.stack(pos, axis=-1))[..., a]
        ua = np.ascontiguousarray(u.transpose(2, 1, 0)).astype(np.float32)                                 # stored z-major, x fastest
        assert ua.shape == np.asarray(sc.vel[a]).shape
        sc.vel[a][:] = ua
        ref.append(ua.ravel())
    return sc, p, ref


# ---- the PCG restated in fp64, and the library's iterate after a whole number of batches -------------------------------------------
# Bounds on max |x_device - x_reference| / max |x_reference| after 25 and 50 iterations (tests/test_gpu_iterates.py): fp64 steps, and the
# Chebyshev polynomial with fp32 inner vectors (its M taken from the device).  About 100x the largest drift measured on an MI355X: 1.3e-13
# (fp64), 1.4e-8 (fp32: the solve's fused first term rounds its fp32 terms differently from the stand-alone apply).  The decomposed solves
# (slabs, bricks, one process per rank: per-rank partial sums and an all-reduce are one more summation order) stay inside that: 5.2e-14 at most.
ITERATE_BOUND = 1e-11
ITERATE_BOUND_F32 = 2e-6
# Cases whose x_50 has converged so far that a 1e-6 error of beta at iteration 24 moves it by less than ITERATE_BOUND (the self-checks,
# tests/test_iterate_tolerances_cpu.py: cavity32 / coil32 Chebyshev-10 1.7e-15 / 5.1e-13, blob6 Chebyshev-4 9.8e-13): x_25 only
ITERATE_SHORT = {("cavity32", "cheb10"): (1,), ("coil32", "cheb10"): (1,), ("blob6", "cheb4"): (1,)}
# cases no bound can check: blob6 Chebyshev-10 has converged by x_25 (the beta error moves it by 3.8e-15)
ITERATE_DROPPED = {("blob6", "cheb10")}
CG_BATCH = 25          # PCG iterations between two stop tests of the library (ps_solve.hip, ps_dist.hpp): an interrupt stops it there


def fdot(a, b):
    """a . b with a correctly rounded sum of the fp64 products (math.fsum): no summation order of a kernel is more accurate"""
    return math.fsum(np.multiply(a, b))


def numpy_pcg(A, M, b, x0, tol, maxit, iters=None, beta_scale=None, on_iterate=None):
    """pcg_external_matrix_A (lib/include/pcg.h:268-340) restated: returns (0-based index of the converged iteration, x).
    iters: stop after exactly that many iterations (x updates) without testing the stop rule, returning (iters, x).
    beta_scale: (i, beta) -> beta, the beta formed at the end of iteration i as the next direction uses it (the tolerance self-checks).
    on_iterate: (k, x) after the k-th x update."""
    x = x0.copy()
    r = b - A(x)
    z = M(r)
    p = z.copy()
    rsold = fdot(r, z)
    n_it = maxit if iters is None else iters
    for i in range(n_it):
        Ap = A(p)
        alpha = rsold / fdot(p, Ap)
        x = x + alpha * p
        if on_iterate is not None:
            on_iterate(i + 1, x)
        r = r - alpha * Ap
        rsnew = fdot(r, r)
        xmag = fdot(x, x)
        rre = rsnew
        if rsnew / xmag < rre:
            rre = rsnew / xmag
        if iters is None and rre < tol * tol:
            return i, x
        z = M(r)
        rsnew = fdot(r, z)
        beta = rsnew / rsold
        if beta_scale is not None:
            beta = beta_scale(i, beta)
        p = z + beta * p
        rsold = rsnew
    return n_it, x


def trajectory_params(p):
    """a copy of params whose stop rule cannot fire within a few hundred iterations: the solve runs until it is interrupted"""
    q = type(p).from_buffer_copy(p)
    q.tolerance = 1e-14
    q.maxSolverIterations = 100000
    return q


def iterate_after(target, m, scene=None, params=None):
    """x (reference numbering) after exactly CG_BATCH * m PCG iterations of a Solver: an interrupt fires at the m-th batch boundary
    (ps_set_interrupt) and the solve returns PS_INCOMPLETE with solveData[1] == CG_BATCH * m.  With scene / params the solver uploads them
    first, with the trajectory tolerance; otherwise it solves what it holds."""
    calls = []
    stop = lambda: calls.append(1) or len(calls) >= m
    if scene is not None:
        target.upload(scene, trajectory_params(params))
    target.set_interrupt(stop)
    try:
        rc = target.step_device()
    finally:
        target.set_interrupt(None)
    assert rc == abi.INCOMPLETE and len(calls) == m, (rc, len(calls))
    assert int(target.stats.solveData[1]) == CG_BATCH * m, target.stats.solveData[1]
    return target.array("solutionVector").copy()


def group_interrupted_step(grp, m, scene, params):
    """Every rank of a Group uploads its part of the scene with the trajectory tolerance; an interrupt on ONE rank, the last, fires at its
    m-th call; the step must return PS_INCOMPLETE after exactly CG_BATCH * m iterations on every rank (Dist::batchEnd carries the request
    to all of them).  The ranks then hold x after that many updates on their owned DOFs (halo entries may be stale: no merge reads them)."""
    calls = []
    stop = lambda: calls.append(1) or len(calls) >= m
    grp.set_scene(scene, trajectory_params(params))
    last = grp.ranks[-1]
    last.set_interrupt(stop)
    try:
        rc = grp.step()
    finally:
        last.set_interrupt(None)
    assert rc == abi.INCOMPLETE and len(calls) == m, (rc, len(calls))
    for r in grp.ranks:                                   # (an in-process group's ranks leave Dist::solve together and share its record)
        assert int(r.stats.result) == abi.INCOMPLETE and int(r.stats.solveData[1]) == CG_BATCH * m, (r.stats.result, r.stats.solveData[1])


def group_iterate_after(grp, m, scene, params, *, numbering):
    """x (the single domain's reference numbering, fp64) after exactly CG_BATCH * m PCG iterations of a decomposed solve on a Group of
    slabs or bricks.  numbering: dof_numbering() of the whole scene"""
    group_interrupted_step(grp, m, scene, params)
    where, n = numbering
    return merged_x(where, n, grp, scene)


# ---- the library's setup and solve against the oracle's, given both (test_gpu_parity.py on the SDF scenes, test_gpu_classification.py on the
# crafted-weight cases): g is a Solver that has uploaded and set up (sc, p), o an Oracle that has run them
def check_tile_blocks(name, sc, p, o, g):
    if o.nRegions == 0:
        pytest.skip("no reduced regions")
    assert np.array_equal(g.array("reducedRegionCOM"), o.array("reducedRegionCOM"))   # exact integer sums
    tol = 1e-12
    assert relerr(g.array("reducedMassMatrices"), o.array("reducedMassMatrices")) < tol
    assert relerr(g.array("reducedViscosityMatrices"), o.array("reducedViscosityMatrices")) < tol
    R = o.nRegions
    # c_fit solves an ill-conditioned LSQ system and BInv inverts B: compare through what they feed
    Mr = o.array("reducedMassMatrices").reshape(R, 26, 26)
    K = o.array("reducedViscosityMatrices").reshape(R, 26, 26)
    Bi = g.array("Inv_Mr_plus_2JDtuDJ").reshape(R, 26, 26)
    Bo = o.array("Inv_Mr_plus_2JDtuDJ").reshape(R, 26, 26)
    for r in range(R):
        B = Mr[r] / sc.dt + 2 * K[r]
        assert np.abs(Bi[r] @ B - np.eye(26)).max() < 1e-7
        assert relerr(Bi[r], Bo[r]) < 1e-6
    assert relerr(g.array("reducedRHSVector"), o.array("reducedRHSVector")) < 1e-8


def check_stencil_blocks(name, sc, p, o, g):
    for nm in ("McInv", "activeRHSVector", "uInv", "pressureRHSVector", "stressRHSVector"):
        assert relerr(g.array(nm), o.array(nm)) < 1e-13, (name, nm)
    G, Dt, JG, JDt = materialise_blocks(g)
    for nm, M in (("G", G), ("Dt", Dt), ("JG", JG), ("JDt", JDt)):
        Mo = o.csr(nm)
        assert M.shape == Mo.shape, (name, nm, M.shape, Mo.shape)
        d = abs(M - Mo)
        scale = abs(Mo).max() if Mo.nnz else 1.0
        assert (d.max() if d.nnz else 0.0) <= 1e-12 * scale, (name, nm)
    # G and Dt have the same sparsity pattern, entry for entry
    assert np.array_equal(G.indptr, o.csr("G").indptr) and np.array_equal(G.indices, o.csr("G").indices)
    S, St = g.S_matrices()
    assert abs(S.T - St).max() == 0.0 if S.nnz else True


def check_rhs_and_operator(name, sc, p, o, g):
    n = o.nP + o.nT
    if n == 0:
        pytest.skip("empty system")
    assert relerr(g.array("b"), o.array("b")) < 1e-9, name
    rng = np.random.RandomState(7)
    for _ in range(2):
        x = rng.randn(n)
        yo, yg = o.apply(x), g.apply(x)
        assert relerr(yg, yo) < 1e-10, name
    # symmetry / definiteness of the device operator itself
    x, y = rng.randn(n), rng.randn(n)
    Ax, Ay = g.apply(x), g.apply(y)
    assert abs(x @ Ay - y @ Ax) < 1e-9 * abs(x @ Ay)
    assert x @ Ax < 0


def check_solve(name, sc, p, o, g):
    rc = g.solve()
    assert rc == o.result, name
    it_o, it_g = o.stats.solveData[1], g.stats.solveData[1]
    assert abs(it_g - it_o) <= max(2, 0.02 * it_o), (name, it_g, it_o)   # CG is order sensitive: +-2 %
    xo, xg = o.array("solutionVector"), g.array("solutionVector")
    if np.linalg.norm(xo) > 0:
        assert np.linalg.norm(xg - xo) <= 10 * p.tolerance * np.linalg.norm(xo), name   # SURVEY §8c tolerance
    vel, valid = g.download()
    for a in range(3):
        assert np.array_equal(valid[a].ravel(), o.array("valid" + "XYZ"[a])), name
        vo = o.array("vel" + "XYZ"[a])
        scale = max(np.abs(vo).max(), 1e-30)
        assert np.abs(vel[a].ravel() - vo).max() <= 20 * p.tolerance * scale, name

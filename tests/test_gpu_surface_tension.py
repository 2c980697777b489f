"""Surface tension (ps_set_surface_tension) on the GPU.

The oracle knows no surface tension, so every check of the new term is a numpy restatement or a closed form: the curvature
(stencil, closest-point sampling, clamp), the impulse in the active and tile right-hand sides and in b, Laplace's law on a resting
droplet, the direction of the flow on an ellipsoid, and the agreement of the other solve routes and the decompositions."""
import numpy as np
import pytest

from polystokes_amd import _abi as abi
from polystokes_amd import scenes
from helpers import basis_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import polystokes_amd
    s = polystokes_amd.Solver(0)
    yield s
    s.close()


def _run(solver, sc, p):
    rc = solver.step(sc, p)
    assert rc == abi.SUCCESS, (rc, solver.last_error())
    return rc


def _active_label(l):
    return (l == abi.ACTIVEFLUID) | (l == abi.BOUNDARY)


# ---- numpy restatements -------------------------------------------------------------------------------------------------
MAX_STEP = 4.0      # cells: the cap of the step to the closest interface point (ps_surface.hip: ST_MAX_STEP)


def _curvature(phi, dx):
    """kappa_c of include/polystokes.h (ps_set_surface_tension): fp64 from the fp32 SDF, kappa stored as fp32, sampled at the closest
    interface point, clamped to [-1/dx, 1/dx], stored as fp32.  phi: (nz, ny, nx)."""
    f = phi.astype(np.float64)
    nz, ny, nx = f.shape
    pad = np.pad(f, 1, mode="edge")                              # indices clamped at the grid border

    def P(di, dj, dk):
        return pad[1 + dk:1 + dk + nz, 1 + dj:1 + dj + ny, 1 + di:1 + di + nx]
    inv = 1.0 / dx
    p0 = P(0, 0, 0)
    px, py, pz = (P(1, 0, 0) - P(-1, 0, 0)) * (0.5 * inv), (P(0, 1, 0) - P(0, -1, 0)) * (0.5 * inv), (P(0, 0, 1) - P(0, 0, -1)) * (0.5 * inv)
    h2, h4 = inv * inv, 0.25 * inv * inv
    pxx, pyy, pzz = (P(1, 0, 0) - 2 * p0 + P(-1, 0, 0)) * h2, (P(0, 1, 0) - 2 * p0 + P(0, -1, 0)) * h2, (P(0, 0, 1) - 2 * p0 + P(0, 0, -1)) * h2
    pxy = (P(1, 1, 0) - P(1, -1, 0) - P(-1, 1, 0) + P(-1, -1, 0)) * h4
    pxz = (P(1, 0, 1) - P(1, 0, -1) - P(-1, 0, 1) + P(-1, 0, -1)) * h4
    pyz = (P(0, 1, 1) - P(0, 1, -1) - P(0, -1, 1) + P(0, -1, -1)) * h4
    g2 = px * px + py * py + pz * pz
    gn = np.sqrt(g2)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = (px * px * (pyy + pzz) + py * py * (pxx + pzz) + pz * pz * (pxx + pyy) - 2 * (px * py * pxy + px * pz * pxz + py * pz * pyz)) / (g2 * gn)
    kraw = np.where(gn >= 1e-6 * inv, k, 0.0).astype(np.float32).astype(np.float64)
    gi = [(P(1, 0, 0) - P(-1, 0, 0)) * 0.5, (P(0, 1, 0) - P(0, -1, 0)) * 0.5, (P(0, 0, 1) - P(0, 0, -1)) * 0.5]
    gg = gi[0] ** 2 + gi[1] ** 2 + gi[2] ** 2
    gn = np.sqrt(gg)
    move = gn >= 1e-6
    with np.errstate(divide="ignore", invalid="ignore"):
        step = np.where(move, -p0 / np.where(move, gg, 1.0), 0.0)
        far = move & (np.abs(p0) > MAX_STEP * gn)                # the step toward the interface is capped at MAX_STEP cells
        step = np.where(far, step * (MAX_STEP * gn / np.where(far, np.abs(p0), 1.0)), step)
    kk, jj, ii = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    lo, hi, t = [], [], []
    for a, (x, n) in enumerate(zip((ii, jj, kk), (nx, ny, nz))):
        u = np.clip(x + step * gi[a], 0.0, n - 1)
        b = np.floor(u).astype(np.int64)
        top = b >= n - 1
        lo.append(np.where(top, n - 1, b))
        hi.append(np.where(top, n - 1, b + 1))
        t.append(np.where(top, 0.0, u - b))
    K = lambda i, j, k: kraw[k, j, i]
    L = lambda a, b, tt: a + (b - a) * tt
    c00 = L(K(lo[0], lo[1], lo[2]), K(hi[0], lo[1], lo[2]), t[0])
    c10 = L(K(lo[0], hi[1], lo[2]), K(hi[0], hi[1], lo[2]), t[0])
    c01 = L(K(lo[0], lo[1], hi[2]), K(hi[0], lo[1], hi[2]), t[0])
    c11 = L(K(lo[0], hi[1], hi[2]), K(hi[0], hi[1], hi[2]), t[0])
    v = L(L(c00, c10, t[1]), L(c01, c11, t[1]), t[2])
    return np.clip(v, -inv, inv).astype(np.float32)


def _ghost_sums(solver, sc):
    """per face grid: sum_c g(f,c) kappa_c from the exported weights, labels and curvature (the impulse is -dt sigma times it)"""
    sh = abi.grid_shapes(sc.nx, sc.ny, sc.nz)
    lab = solver.array("centerLabels").reshape(sh["center"])
    lw = solver.array("centerLiquidWeights").reshape(sh["center"]).astype(np.float64)
    kap = solver.array("surfaceCurvature").reshape(sh["center"]).astype(np.float64)
    ghost = np.where(_active_label(lab) | (lab == abi.REDUCED), 1.0 - lw, 1.0) * kap
    out = []
    for a in range(3):
        ax = 2 - a
        wf = solver.array("face" + "XYZ"[a] + "FluidWeights").reshape(sh["face" + "XYZ"[a]]).astype(np.float64)
        zero = np.zeros_like(np.take(ghost, [0], axis=ax))
        lower = np.concatenate([zero, ghost], axis=ax)           # cell f - 1 (none below face 0)
        upper = np.concatenate([ghost, zero], axis=ax)           # cell f (none above the last face)
        out.append(wf * (upper - lower) / sc.dx)
    return out


def _per_row(solver, per_face):
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


def _reduced_impulse(solver, sc, sums, sigma):
    """sum over each region's reduced faces of C_f^T (-dt sigma sum_c g kappa), and the number of faces with a non-zero impulse"""
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
        np.add.at(out, r, C * (-sc.dt * sigma * sums[a][k, j, i])[:, None])
    return out, hits


def _delta_b(solver, sc, d_rhs_a, d_rhs_r):
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


def _check_rhs_and_b(solver, sc, sigma, before, expect_reduced):
    """the active rhs, the tiles' rhs and b after a sigma > 0 setup, against their sigma = 0 values `before` and the numpy restatement"""
    rhs0, rr0, b0 = before
    rhs1, rr1, b1 = solver.array("activeRHSVector"), solver.array("reducedRHSVector"), solver.array("b")
    sums = _ghost_sums(solver, sc)
    want = -sc.dt * sigma * _per_row(solver, sums)
    assert np.abs(want).max() > 1.0
    assert np.abs((rhs1 - rhs0) - want).max() <= 1e-12 * max(np.abs(rhs1).max(), np.abs(want).max())
    red, hits = _reduced_impulse(solver, sc, sums, sigma)
    assert int(solver.array("surfaceTensionReducedFaces")[0]) == hits
    assert (hits > 0) == expect_reduced, hits
    assert np.abs((rr1 - rr0) - red.ravel()).max() <= 1e-12 * max(np.abs(rr1).max(), np.abs(red).max(), 1e-300)
    db = _delta_b(solver, sc, want, red.ravel())
    assert np.abs((b1 - b0) - db).max() <= 1e-12 * max(np.abs(b1).max(), np.abs(db).max())
    return hits


# ---- 1. API ---------------------------------------------------------------------------------------------------------------
def test_setting_errors_and_persistence():
    import polystokes_amd
    s = polystokes_amd.Solver(0)
    try:
        sc, p = scenes.droplet(24)
        assert s.set_surface_tension(0.5) == abi.SUCCESS
        for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
            assert s.set_surface_tension(bad) == abi.INVALID, bad
            assert "ps_set_surface_tension" in s.last_error()
        _run(s, sc, p)                                            # the setting survives the upload inside polystokes_step
        assert float(s.array("surfaceTension")[0]) == 0.5
        assert s.array("surfaceCurvature").size == sc.nx * sc.ny * sc.nz
        assert s.set_surface_tension(0.0) == abi.SUCCESS
        _run(s, sc, p)
        assert float(s.array("surfaceTension")[0]) == 0.0
        with pytest.raises(KeyError):
            s.array("surfaceCurvature")
    finally:
        s.close()


# ---- 2. curvature ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blob", "droplet48"])
def test_curvature_against_numpy(gpu, name):
    sc, p = scenes.blob(seed=2) if name == "blob" else scenes.droplet(48)
    gpu.set_surface_tension(0.07)
    try:
        _run(gpu, sc, p)
        got = gpu.array("surfaceCurvature").reshape(sc.surface.shape)
    finally:
        gpu.set_surface_tension(0.0)
    ref = _curvature(sc.surface, sc.dx)
    assert np.abs(got - ref).max() <= 1e-5 / sc.dx, np.abs(got - ref).max() * sc.dx
    assert np.abs(got).max() <= np.float32(1.0 / sc.dx)
    if name == "droplet48":
        R = 0.33
        near = np.abs(sc.surface) < sc.dx
        assert near.sum() > 1000
        assert np.abs(got[near] * R / 2 - 1).max() <= 0.02, np.abs(got[near] * R / 2 - 1).max()


# ---- 3. right-hand sides --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blob", "droplet"])
def test_rhs_against_numpy(gpu, name):
    sc, p = scenes.blob(seed=1) if name == "blob" else scenes.droplet(32)
    sigma = 50.0
    gpu.set_surface_tension(0.0)
    _run(gpu, sc, p)
    before = gpu.array("activeRHSVector"), gpu.array("reducedRHSVector"), gpu.array("b")
    gpu.set_surface_tension(sigma)
    try:
        _run(gpu, sc, p)
        # even with the default layers some tile faces touch a boundary cell with liquidW < 1 (56 on the blob, 192 on the droplet):
        # b is restated with the tile term
        _check_rhs_and_b(gpu, sc, sigma, before, expect_reduced=True)
    finally:
        gpu.set_surface_tension(0.0)


def test_reduced_faces_next_to_the_surface(gpu):
    """with no active liquid boundary layer the tiles reach the surface: reduced faces get the impulse through C_f^T"""
    sc, p = scenes.droplet(32)
    p.activeLiquidBoundaryLayerSize, p.tilePadding = 0, 1
    sigma = 20.0
    gpu.set_surface_tension(0.0)
    _run(gpu, sc, p)
    before = gpu.array("activeRHSVector"), gpu.array("reducedRHSVector"), gpu.array("b")
    gpu.set_surface_tension(sigma)
    try:
        _run(gpu, sc, p)
        _check_rhs_and_b(gpu, sc, sigma, before, expect_reduced=True)
    finally:
        gpu.set_surface_tension(0.0)


# ---- 4. Laplace's law -----------------------------------------------------------------------------------------------------
# Measured on an MI355X (profiles/surface_tension.md), n = 48, sigma = 1: mean interior pressure error 0.005 %, spurious max|u| / U = 4.09 %
# (8.43 / 4.09 / 2.09 % at n = 32 / 48 / 64: first order in dx, at the interface).  The issue's unmeasured targets were 2 % for both; the
# committed bounds are the measured values with margin: 0.1 % (20x) for the pressure, 6 % (1.5x) for the velocity.
LAPLACE_P_TOL = 0.001
LAPLACE_U_TOL = 0.06
# With the tiles at the surface (activeLiquidBoundaryLayerSize = 0, tilePadding = 1), n = 48: measured 0.002 % and 2.54 % (8.43 / 2.54 / 1.92 %
# at n = 32 / 48 / 64); committed 0.1 % and 4 % (1.6x).
LAPLACE_TILES_P_TOL = 0.001
LAPLACE_TILES_U_TOL = 0.04


def laplace(n, sigma=1.0, radius=0.33, tol=1e-8, liquid_layers=None, pad=2):
    """(relative error of the mean interior pressure against 2 sigma / R, max|u| / (dt sigma (2/R) / (rho dx)), iterations);
    liquid_layers = activeLiquidBoundaryLayerSize (None: the default 2)"""
    import polystokes_amd
    sc, p = scenes.droplet(n, radius=radius, pad=pad)
    sc.surface_tension = sigma
    p.tolerance, p.maxSolverIterations = tol, 50000
    if liquid_layers is not None:
        p.activeLiquidBoundaryLayerSize = liquid_layers
    s = polystokes_amd.Solver(0)
    try:
        _run(s, sc, p)
        pr = s.solution_fields()["pressure"]
        lab = s.array("centerLabels").reshape(pr.shape)
        inner = (sc.surface < -3 * sc.dx) & _active_label(lab)
        assert inner.sum() > 100
        pe = abs(pr[inner].astype(np.float64).mean() / (2 * sigma / radius) - 1)
        U = sc.dt * sigma * (2 / radius) / (sc.density * sc.dx)
        umax = max(np.abs(v).max() for v in s.vel)
        return pe, umax / U, int(s.stats.solveData[1])
    finally:
        s.close()


def test_laplace_law_resting_droplet():
    pe, ur, _ = laplace(48)
    assert pe <= LAPLACE_P_TOL, pe
    assert ur <= LAPLACE_U_TOL, ur


def test_laplace_law_with_tiles_at_the_surface():
    """activeLiquidBoundaryLayerSize = 0, padding 1: the tiles reach the free surface, so reduced faces carry the jump and reduced cells
    with liquidW < 1 take the ghost pressure on their non-liquid part only.  The droplet must still rest at the Laplace pressure."""
    pe, ur, _ = laplace(48, liquid_layers=0, pad=1)
    assert pe <= LAPLACE_TILES_P_TOL, pe
    assert ur <= LAPLACE_TILES_U_TOL, ur


# ---- 5. direction ---------------------------------------------------------------------------------------------------------
def test_ellipsoid_flows_from_tips_to_equator(gpu):
    n = 32
    sc, p = scenes.ellipsoid_droplet(n, axes=(0.36, 0.26, 0.26), sigma=1.0)
    p.tolerance = 1e-8
    try:
        _run(gpu, sc, p)
        vx, vy, vz = gpu.vel
        c = [n // 2 - 1, n // 2]                                   # the two cell layers around the centre plane
        tip_hi = vx[:, :, 25:28][c][:, c].mean()                   # x faces inside the tip at x = 0.86
        tip_lo = vx[:, :, 5:8][c][:, c].mean()                     # ... and at x = 0.14
        assert tip_hi < 0 < tip_lo, (tip_hi, tip_lo)
        end_hi = vy[:, 22:25, :][c][:, :, c].mean()                # y faces inside the end of the short axis at y = 0.76
        end_lo = vy[:, 8:11, :][c][:, :, c].mean()
        assert end_lo < 0 < end_hi, (end_lo, end_hi)
        endz = vz[22:25][:, c][:, :, c].mean()
        assert endz > 0
        pr = gpu.solution_fields()["pressure"]
        lab = gpu.array("centerLabels").reshape(pr.shape)
        x, y, z = [(np.arange(n) + 0.5) / n - 0.5 for _ in range(3)]
        Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
        use = _active_label(lab) & (sc.surface < -sc.dx)
        tips = use & (np.abs(X) > 0.25)
        equator = use & (np.abs(X) < 0.06) & (np.hypot(Y, Z) > 0.16)
        assert tips.sum() > 20 and equator.sum() > 20
        assert pr[tips].mean() > pr[equator].mean(), (pr[tips].mean(), pr[equator].mean())
    finally:
        gpu.set_surface_tension(0.0)


# ---- 6. no free surface, no force; sigma = 0 is the default path ---------------------------------------------------------
def test_cavity_is_unchanged(gpu):
    sc, p = scenes.cavity(32)
    gpu.set_surface_tension(0.0)
    _run(gpu, sc, p)
    v0 = [v.copy() for v in gpu.vel]
    gpu.set_surface_tension(3.0)
    try:
        _run(gpu, sc, p)
        assert float(gpu.array("surfaceTension")[0]) == 3.0
        for a in range(3):
            assert np.array_equal(gpu.vel[a], v0[a])
    finally:
        gpu.set_surface_tension(0.0)


def test_zero_sigma_is_the_default_path():
    import polystokes_amd
    sc, p = scenes.droplet(32)
    sc.vel[1][:] = -0.3                                             # something to project
    a = polystokes_amd.Solver(0)
    b = polystokes_amd.Solver(0)
    try:
        _run(a, sc, p)
        assert b.set_surface_tension(2.0) == abi.SUCCESS and b.set_surface_tension(0.0) == abi.SUCCESS
        _run(b, sc, p)
        for q in range(3):
            assert np.array_equal(a.vel[q], b.vel[q])
        for name in ("activeRHSVector", "b", "solutionVector", "reducedRHSVector"):
            assert np.array_equal(a.array(name), b.array(name)), name
        assert float(a.array("surfaceTension")[0]) == 0.0 and float(b.array("surfaceTension")[0]) == 0.0
    finally:
        a.close()
        b.close()


# ---- 7. other routes ------------------------------------------------------------------------------------------------------
def test_exported_system_solves_the_same(gpu, tmp_path):
    import scipy.io
    sc, p = scenes.droplet(32)
    p.tolerance, p.maxSolverIterations, p.preconditioner = 1e-8, 20000, abi.PRE_DIAGONAL
    gpu.set_surface_tension(1.0)
    try:
        _run(gpu, sc, p)
        pre = str(tmp_path) + "/st."
        gpu.export_component_matrices(pre)
        x_mem = np.asarray(scipy.io.mmread(pre + "solutionVector.mtx")).ravel()
        rc, x = gpu.solve_exported_system(pre, p, sc.dt, x_mem.size)
        assert rc == abi.SUCCESS
        # measured 6.2 tol: the files carry 17 digits and the two PCGs sum in different orders
        assert np.linalg.norm(x - x_mem) <= 10 * p.tolerance * np.linalg.norm(x_mem)
    finally:
        gpu.set_surface_tension(0.0)


def test_preconditioners_and_warm_start_agree(gpu):
    import polystokes_amd
    sc, p = scenes.droplet(32)
    sc.surface_tension = 1.0
    p.tolerance = 1e-8
    xs = {}
    try:
        for pre in (abi.PRE_DIAGONAL, abi.PRE_CHEBYSHEV_F32):
            p.preconditioner = pre
            _run(gpu, sc, p)
            xs[pre] = gpu.array("solutionVector")
    finally:
        gpu.set_surface_tension(0.0)                          # (the scene set it on the module's solver)
    x = xs[abi.PRE_DIAGONAL]
    # The stop rule bounds the residual, not the error: on this stiff scene (viscosity 50, sigma 1) the two solutions measured 51 tol apart
    # in norm and 138 tol in the largest entry, at tolerance 1e-6 and 1e-8 alike (profiles/surface_tension.md).
    assert np.linalg.norm(xs[abi.PRE_CHEBYSHEV_F32] - x) <= 100 * p.tolerance * np.linalg.norm(x)
    assert np.abs(xs[abi.PRE_CHEBYSHEV_F32] - x).max() <= 300 * p.tolerance * np.abs(x).max()
    w = polystokes_amd.Solver(0)
    try:
        p.preconditioner = abi.PRE_DIAGONAL
        w.set_warm_start(1)
        _run(w, sc, p)
        cold_it = w.stats.solveData[1]
        _run(w, sc, p)
        assert int(w.array("warmStartUsed")[0]) == 1
        assert w.stats.solveData[1] < cold_it
        assert np.linalg.norm(w.array("solutionVector") - x) <= 100 * p.tolerance * np.linalg.norm(x)
    finally:
        w.close()


# ---- 8. decompositions ----------------------------------------------------------------------------------------------------
def _liquid_under_ceiling(n=64, ceiling=40):
    """a liquid layer hanging from a solid ceiling (no gravity): solid above the face plane z = ceiling, liquid from there down to a wavy
    free surface near z = 10 cells.  The faces on the ceiling plane are open; their upper cells are solid cells without a pressure DOF that
    carry the whole ghost coefficient, and the liquid SDF puts their closest interface point about 30 cells below them — beyond the halo
    block of a rank that owns the ceiling when the grid is cut at z = 32.  Their step to the interface is capped (ps_surface.hip)."""
    sc, p = scenes.droplet(n, tile=8)
    x = (np.arange(n) + 0.5) / n
    z = (np.arange(n) + 0.5) * sc.dx
    h = (10 + 4 * np.cos(2 * np.pi * x)[None, :, None] * np.cos(2 * np.pi * x)[None, None, :]) * sc.dx
    sc.surface[:] = (h - z[:, None, None]).astype(np.float32)
    sc.collision[:] = np.broadcast_to((ceiling * sc.dx - z).astype(np.float32)[:, None, None], sc.collision.shape)
    return sc, p


def _owned_boxes(world, dims, sc, p):
    """per rank: (local slices of the owned cells, global slices of the same cells)"""
    from polystokes_amd import partition
    out = []
    for r in range(world):
        if dims is None:
            sl = partition.make_slab(sc.nz, world, r, p.tileSize)
            out.append(((slice(sl.zLoOwned, sl.zHiOwned), slice(None), slice(None)),
                        (slice(sl.g0 + sl.zLoOwned, sl.g0 + sl.zHiOwned), slice(None), slice(None))))
        else:
            b = partition.make_brick((sc.nx, sc.ny, sc.nz), dims, r, p.tileSize)
            loc = tuple(slice(b.lo[a], b.hi[a]) for a in (2, 1, 0))
            glob = tuple(slice(b.origin[a] + b.lo[a], b.origin[a] + b.hi[a]) for a in (2, 1, 0))
            out.append((loc, glob))
    return out


@pytest.mark.parametrize("dims", [None, (2, 2, 2)])
@pytest.mark.parametrize("scene", ["droplet", "liquid_under_ceiling"])
def test_decompositions_match_single_domain(dims, scene):
    import polystokes_amd
    world = 2 if dims is None else 8
    sc, p = scenes.droplet(32, tile=8) if scene == "droplet" else _liquid_under_ceiling()
    sc.vel[1][:] = -0.2
    sc.surface_tension = 1.0
    single = polystokes_amd.Solver(0)
    grp = polystokes_amd.Group(world, dims=dims)
    try:
        _run(single, sc, p)
        assert float(single.array("surfaceTension")[0]) == 1.0
        kap = single.array("surfaceCurvature").reshape(sc.surface.shape)
        if scene == "liquid_under_ceiling":
            lab = single.array("centerLabels").reshape(sc.surface.shape)
            row = single.array("faceRowZ").reshape(sc.nz + 1, sc.ny, sc.nx)
            deep = (lab[40] == abi.SOLID) & (row[40] >= 0) & (sc.surface[40] < -16 * sc.dx) & (kap[40] != 0)
            assert deep.sum() > 1000, deep.sum()
        rc = grp.solve_scene(sc, p)
        assert rc == abi.SUCCESS
        for r in grp.ranks:
            assert float(r.array("surfaceTension")[0]) == 1.0
        # every rank computes the single domain's kappa_c on the cells it owns
        for r, (loc, glob) in zip(grp.ranks, _owned_boxes(world, dims, sc, p)):
            sh = abi.grid_shapes(r.scene.nx, r.scene.ny, r.scene.nz)["center"]
            assert np.array_equal(r.array("surfaceCurvature").reshape(sh)[loc], kap[glob])
        for a in range(3):
            assert np.array_equal(grp.valid[a], single.valid[a])
            scale = max(np.abs(single.vel[a]).max(), 1e-30)
            assert np.abs(grp.vel[a] - single.vel[a]).max() <= 20 * p.tolerance * scale
    finally:
        grp.close()
        single.close()

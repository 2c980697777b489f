"""Variable density (ps_upload_density_field) on the GPU.

The oracle knows one scalar density, so the density-dependent assembly is checked against numpy restatements: the face mass
(McInv, Mc, the active rhs) face by face, the tile mass Mr = sum_f rho_f C_f^T C_f region by region, and then the operator and
solve against the literal path of the exported component matrices.  A constant field is the scalar path bit for bit."""
import numpy as np
import pytest

from polystokes_amd import _abi as abi
from polystokes_amd import scenes
from helpers import basis_rows, per_row, rigid_rotation_scene

import children

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import polystokes_amd
    s = polystokes_amd.Solver(0)
    yield s
    s.close()


def _scene(name, kind=None, **kw):
    """(scene, params) with an optional density field; the cavity (density 1) gets rho0 = 4 so that the field lies inside [1, 1e5]"""
    if name == "blob":
        sc, p = scenes.blob(seed=kw.pop("seed", 0))
        rho0 = None
    else:
        sc, p = scenes.cavity(int(name[6:]))
        rho0 = 4.0 if kind == "smooth" else 2.0
    if kind is not None:
        scenes.with_density_field(sc, kind, rho0=rho0)
    return sc, p


def _face_density(sc, p):
    """numpy restatement of the face sampler (include/polystokes.h, ps_upload_density_field): per axis, the clamped fp32 face density"""
    f = sc.density_field
    out = []
    for a in range(3):
        ax = 2 - a                                  # numpy axis of grid axis a (arrays are (z, y, x))
        lo = np.concatenate([np.take(f, [0], axis=ax), f], axis=ax)
        hi = np.concatenate([f, np.take(f, [f.shape[ax] - 1], axis=ax)], axis=ax)
        r = lo + (hi - lo) * np.float32(0.5)
        # faces on the grid boundary take their one cell
        idx = [slice(None)] * 3
        idx[ax] = 0
        r[tuple(idx)] = f[tuple(idx)]
        idx[ax] = -1
        sl = [slice(None)] * 3
        sl[ax] = -1
        r[tuple(idx)] = f[tuple(sl)]
        out.append(np.clip(r.astype(np.float64), p.mindensity, p.maxdensity))
    return out


def _run(solver, sc, p):
    rc = solver.step(sc, p)
    assert rc == abi.SUCCESS, (rc, solver.last_error())
    return rc


# ---- 1. API --------------------------------------------------------------------------------------------------------------
def test_api_errors_and_drops():
    import polystokes_amd
    s = polystokes_amd.Solver(0)
    try:
        field = np.ones((8, 8, 8), np.float32)
        assert s.L.ps_upload_density_field(s.h, field.ctypes.data) == abi.INVALID       # before any upload
        assert "ps_upload_fields" in s.last_error()
        sc, p = _scene("cavity32")
        s.upload(sc, p)
        bad = np.full((sc.nz, sc.ny, sc.nx), 3.0, np.float32)
        bad[5, 6, 7] = np.nan
        assert s.upload_density_field(bad) == abi.INVALID
        assert "non-finite" in s.last_error()
        bad[5, 6, 7] = np.inf
        assert s.upload_density_field(bad) == abi.INVALID
        for lo, hi in ((0.0, 10.0), (-1.0, 10.0), (5.0, 4.0), (1.0, float("inf")), (float("nan"), 10.0)):
            q = abi.default_params(mindensity=lo, maxdensity=hi)
            s.upload(sc, q)
            assert s.upload_density_field(np.full((sc.nz, sc.ny, sc.nx), 3.0, np.float32)) == abi.INVALID, (lo, hi)
            assert "mindensity" in s.last_error()
        # a valid field is used; NULL drops it; a second upload drops it
        scf, p = _scene("cavity32", "smooth")
        s.upload(scf, p)
        assert s.setup() == abi.SUCCESS and int(s.array("densityField")[0]) == 1
        assert s.upload_density_field(None) == abi.SUCCESS
        assert int(s.array("densityField")[0]) == 0
        assert s.setup() == abi.SUCCESS and int(s.array("densityField")[0]) == 0
        s.upload(scf, p)
        assert s.setup() == abi.SUCCESS and int(s.array("densityField")[0]) == 1
        s.upload(sc, p)                                    # no field passed again
        assert s.setup() == abi.SUCCESS and int(s.array("densityField")[0]) == 0
        # a constant field is the scalar path, not a field
        scc, p = _scene("cavity32")
        scc.density_field = np.full((sc.nz, sc.ny, sc.nx), 3.0, np.float32)
        s.upload(scc, p)
        assert s.setup() == abi.SUCCESS and int(s.array("densityField")[0]) == 0
    finally:
        s.close()


# ---- 2. a constant field is the scalar path ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cavity32", "blob0", "blob1", "blob2"])
@pytest.mark.parametrize("precond", [abi.PRE_DIAGONAL, abi.PRE_CHEBYSHEV_F32])
def test_constant_field_equals_scalar(gpu, name, precond):
    def run(density, field, lo=1.0, hi=100000.0):
        sc, p = _scene(name if name.startswith("cavity") else "blob", seed=int(name[4:]) if name.startswith("blob") else 0)
        p.preconditioner, p.exportComponentMatrices, p.mindensity, p.maxdensity = precond, 1, lo, hi
        sc.density = density
        if field is not None:
            sc.density_field = np.full((sc.nz, sc.ny, sc.nx), field, np.float32)
        _run(gpu, sc, p)
        return dict(vel=[v.copy() for v in gpu.vel], valid=[v.copy() for v in gpu.valid], x=gpu.array("solutionVector"),
                    Mc=gpu.array("Mc"), Mr=gpu.array("reducedMassMatrices"), it=gpu.stats.solveData[1],
                    df=int(gpu.array("densityField")[0]))
    v = 3.0 if name.startswith("cavity") else 450.0
    cases = [(v, v, 1.0, 1e5), (1.0, 0.25, 1.0, 1e5), (100000.0, 2.5e5, 1.0, 1e5), (2.0, 1.0, 2.0, 8.0)]
    for scalar, const, lo, hi in cases:
        a = run(scalar, None, lo, hi)
        b = run(17.0, const, lo, hi)                       # the scalar of the upload is replaced by clamp(const)
        assert b["df"] == 0
        for k in ("x", "Mc", "Mr"):
            assert a[k].tobytes() == b[k].tobytes(), (name, k, scalar)
        for q in range(3):
            assert a["vel"][q].tobytes() == b["vel"][q].tobytes() and a["valid"][q].tobytes() == b["valid"][q].tobytes()
        assert a["it"] == b["it"]


# ---- 3. face mass against numpy --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blob", "cavity48"])
@pytest.mark.parametrize("kind", ["smooth", "layers"])
def test_face_mass_against_numpy(gpu, name, kind):
    _check_face_mass(gpu, name, kind, None)


def test_face_mass_with_custom_clamp(gpu):
    _check_face_mass(gpu, "cavity48", "smooth", (3.0, 5.0))


def _check_face_mass(gpu, name, kind, clamp):
    sc1, p = _scene(name)
    p.exportComponentMatrices = 1
    sc1.density = 1.0
    _run(gpu, sc1, p)
    mc1, rhs1 = gpu.array("Mc"), gpu.array("activeRHSVector")
    sc, p = _scene(name, kind)
    p.exportComponentMatrices = 1
    if clamp is not None:
        p.mindensity, p.maxdensity = clamp
    _run(gpu, sc, p)
    assert int(gpu.array("densityField")[0]) == 1
    rho = per_row(gpu, _face_density(sc, p))
    if clamp is not None:
        assert (rho == clamp[0]).any() and (rho == clamp[1]).any() and ((rho > clamp[0]) & (rho < clamp[1])).any()
    mc, mcinv, rhs = gpu.array("Mc"), gpu.array("McInv"), gpu.array("activeRHSVector")
    assert np.abs(mc / mc1 / rho - 1).max() <= 2.4e-7
    assert np.abs(mcinv * mc - 1).max() <= 1e-15
    nz = np.abs(rhs1) > 0
    assert nz.sum() > 10
    assert np.abs(rhs[nz] / rhs1[nz] / rho[nz] - 1).max() <= 2.4e-7
    assert np.array_equal(rhs[~nz], rhs1[~nz])
    if kind == "smooth":
        assert len(np.unique(mcinv)) > 256


# ---- 4. tile mass against numpy ------------------------------------------------------------------------------------------
def _tile_mass(solver, sc, rho_faces):
    """rho_f-weighted sum of C_f^T C_f over each region's mass faces (ps_tiles.hip MODE_MASS: a face of the region whose upper cell is
    reduced, or whose lower cell is reduced and upper cell active)"""
    R = solver.nRegions
    sh = abi.grid_shapes(sc.nx, sc.ny, sc.nz)
    lab = solver.array("centerLabels").reshape(sh["center"])
    com = solver.array("reducedRegionCOM").reshape(-1, 3)
    active = lambda l: (l == abi.ACTIVEFLUID) | (l == abi.BOUNDARY)
    offs, axes, regs, rhos = [], [], [], []
    for a in range(3):
        red = solver.array("face" + "XYZ"[a] + "ReducedIndices").reshape(sh["face" + "XYZ"[a]])
        k, j, i = np.nonzero(red >= 0)
        idx = [i, j, k]
        hi = lab[np.minimum(k, sc.nz - 1), np.minimum(j, sc.ny - 1), np.minimum(i, sc.nx - 1)]
        inside_hi = idx[a] < [sc.nx, sc.ny, sc.nz][a]
        hi = np.where(inside_hi, hi, abi.UNASSIGNED)
        lo_idx = [i.copy(), j.copy(), k.copy()]
        lo_idx[a] = lo_idx[a] - 1
        lo = lab[np.maximum(lo_idx[2], 0), np.maximum(lo_idx[1], 0), np.maximum(lo_idx[0], 0)]
        lo = np.where(lo_idx[a] >= 0, lo, abi.UNASSIGNED)
        use = (hi == abi.REDUCED) | ((lo == abi.REDUCED) & active(hi))
        pos = np.stack([i, j, k], axis=1).astype(np.float64)[use]
        pos[:, a] -= 0.5
        r = red[k, j, i][use]
        offs.append(pos * sc.dx - com[r])
        axes.append(np.full(len(r), a))
        regs.append(r)
        rhos.append(rho_faces[a][k, j, i][use])
    off, ax, reg, rho = (np.concatenate(v) for v in (offs, axes, regs, rhos))
    C = basis_rows(off, ax)
    Mr = np.zeros((R, 26, 26))
    for r in range(R):
        m = reg == r
        Mr[r] = C[m].T @ (rho[m, None] * C[m])
    return Mr


def _check_tile_mass(gpu, name, kind):
    sc, p = _scene(name)
    _run(gpu, sc, p)
    assert gpu.nRegions >= 2
    sh = abi.grid_shapes(sc.nx, sc.ny, sc.nz)
    const = [np.full(sh["face" + "XYZ"[a]], float(np.float32(sc.density))) for a in range(3)]
    ref = _tile_mass(gpu, sc, const)
    got = gpu.array("reducedMassMatrices").reshape(ref.shape)
    scale = np.abs(ref).max()
    assert np.abs(got - ref).max() <= 1e-12 * scale, "scalar face set"
    sc, p = _scene(name, kind)
    _run(gpu, sc, p)
    ref = _tile_mass(gpu, sc, _face_density(sc, p))
    got = gpu.array("reducedMassMatrices").reshape(ref.shape)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    cfit = gpu.array("reducedRegionBestFitVectors").reshape(-1, 26)
    rhs = gpu.array("reducedRHSVector").reshape(-1, 26)
    want = np.einsum("rij,rj->ri", got, cfit)
    assert np.abs(rhs - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300)


@pytest.mark.parametrize("name,kind", [("blob", "smooth"), ("cavity32", "layers")])
def test_tile_mass_against_numpy(gpu, name, kind):
    _check_tile_mass(gpu, name, kind)


def test_tile_mass_valu_form(tmp_path):
    """the VALU form of the tile sums (PS_TILE_VALU=1, read once per process): a child runs the same checks"""
    code = ("import test_gpu_variable_density as t\n"
            "s = polystokes_amd.Solver(0)\n"
            "t._check_tile_mass(s, 'blob', 'smooth'); t._check_tile_mass(s, 'cavity32', 'layers')\n"
            "s.close(); print('VALU_OK')\n")
    pr = children.run_python(code, limit=300, env={"PS_TILE_VALU": "1"})
    assert "VALU_OK" in pr.stdout, pr.describe()


# ---- 5. operator and solve against the literal path ---------------------------------------------------------------------
def test_exported_field_system_solves_the_same(gpu, tmp_path):
    import scipy.io
    sc, p = _scene("blob", "smooth")
    p.tolerance, p.maxSolverIterations, p.preconditioner = 1e-8, 20000, abi.PRE_DIAGONAL
    _run(gpu, sc, p)
    its = gpu.stats.solveData[1]
    pre = str(tmp_path) + "/field."
    gpu.export_component_matrices(pre)
    x_mem = np.asarray(scipy.io.mmread(pre + "solutionVector.mtx")).ravel()
    mcinv = np.asarray(scipy.io.mmread(pre + "Mat_McInv.mtx").diagonal()).ravel()
    assert np.abs(mcinv / gpu.array("McInv") - 1).max() <= 1e-15
    rc, x = gpu.solve_exported_system(pre, p, sc.dt, x_mem.size)
    assert rc == abi.SUCCESS
    assert abs(gpu.stats.solveData[1] - its) <= max(2, 0.02 * its)
    # (the bound of test_exported_system_import_and_solve: the files carry 17 digits, the two PCGs sum in different orders)
    assert np.linalg.norm(x - x_mem) <= 1e-6 * np.linalg.norm(x_mem)


def test_eigen_solver_on_a_field_scene(gpu):
    """solverType = EIGEN stops on ||r|| < tol ||b||, the PCG on the reference's rre: at tol 1e-11 both sit within 1e-6 of the solution"""
    sc, p = _scene("blob", "layers")
    p.tolerance, p.maxSolverIterations = 1e-11, 50000
    _run(gpu, sc, p)
    x_pcg = gpu.array("solutionVector")
    p.solverType = abi.EIGEN
    rc = gpu.step(sc, p)
    assert rc == abi.SUCCESS
    assert int(gpu.array("densityField")[0]) == 1
    x_e = gpu.array("solutionVector")
    assert np.abs(x_e - x_pcg).max() <= 1e-6 * np.abs(x_pcg).max()


# ---- 6. the fast path: two-unit S kernel with the fp64 face mass ----------------------------------------------------------
_CHILD = ("sc, p = scenes.cavity(80)\nscenes.with_density_field(sc, 'smooth', rho0=4.0)\n"
          "p.preconditioner = {pre}\np.tolerance = 1e-6\n"
          "s = polystokes_amd.Solver(0)\nrc = s.step(sc, p)\n"
          "np.save({out!r}, s.array('solutionVector'))\n"
          "print('RESULT ' + json.dumps(dict(rc=rc, it=s.stats.solveData[1], dc=int(s.array('diagonalsCoded')[0]), c32=int(s.array('chebInner32')[0]),"
          " fused=int(s.array('fusedStep')[0]))))\n")


def _child(tmp_path, tag, env, pre=abi.PRE_CHEBYSHEV_F32):
    out = str(tmp_path / (tag + ".npy"))
    info = children.run_python(_CHILD.format(pre=pre, out=out), limit=300, env=env).result()
    assert info["rc"] == abi.SUCCESS, (tag, info)
    return info, np.load(out)


def test_fast_path_with_uncoded_face_mass(tmp_path):
    base, x = _child(tmp_path, "dual", {})
    assert base["dc"] & 2 == 0                       # McInv is not value-set coded
    assert base["c32"] == 1                          # the fp32 polynomial runs on the uncoded face mass
    tol = 10 * 1e-6 * np.abs(x).max()
    _, x64 = _child(tmp_path, "cheb64", {}, pre=abi.PRE_CHEBYSHEV)
    _, xj = _child(tmp_path, "jacobi", {}, pre=abi.PRE_DIAGONAL)
    assert np.abs(x - x64).max() <= tol and np.abs(x - xj).max() <= tol
    one, x1 = _child(tmp_path, "one_unit", {"PS_S_DUAL": "0"})
    assert one["c32"] == 0                           # (the fp32 polynomial needs the two-unit kernels)
    assert np.abs(x - x1).max() <= tol
    onej, x1j = _child(tmp_path, "one_unit_jacobi", {"PS_S_DUAL": "0"}, pre=abi.PRE_DIAGONAL)
    dualj, x2j = _child(tmp_path, "dual_jacobi", {}, pre=abi.PRE_DIAGONAL)
    assert abs(onej["it"] - dualj["it"]) <= max(2, 0.02 * dualj["it"])
    assert np.abs(x1j - x2j).max() <= tol
    for fused in ("1", "0"):
        info, xf = _child(tmp_path, "fused" + fused, {"PS_FUSED_R": fused}, pre=abi.PRE_DIAGONAL)
        assert info["fused"] == int(fused)
        assert abs(info["it"] - dualj["it"]) <= max(2, 0.02 * dualj["it"])
        assert np.abs(xf - x2j).max() <= tol


# ---- 7. decompositions -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [None, (2, 2, 2)])
def test_decompositions_match_single_domain(dims):
    import polystokes_amd
    if dims is None:
        world = 2
    else:
        world = 8
    sc, p = scenes.cavity(64)
    scenes.with_density_field(sc, "smooth", rho0=4.0)
    single = polystokes_amd.Solver(0)
    _run(single, sc, p)
    assert int(single.array("densityField")[0]) == 1
    grp = polystokes_amd.Group(world, dims=dims)
    rc = grp.solve_scene(sc, p)
    assert rc == abi.SUCCESS
    for r in grp.ranks:
        assert int(r.array("densityField")[0]) == 1
    it1, it2 = single.stats.solveData[1], grp.stats.solveData[1]
    assert abs(it1 - it2) <= max(2, 0.02 * it1), (it1, it2)
    for a in range(3):
        assert np.array_equal(grp.valid[a], single.valid[a])
        scale = max(np.abs(single.vel[a]).max(), 1e-30)
        assert np.abs(grp.vel[a] - single.vel[a]).max() <= 20 * p.tolerance * scale
    grp.close()
    single.close()


# ---- 8. rigid motion ----------------------------------------------------------------------------------------------------
def test_rigid_motion_with_layered_density(gpu):
    sc, p, ref = rigid_rotation_scene()
    for a in range(3):                                # plus a translation
        sc.vel[a] += np.float32(0.1 * (a + 1))
        ref[a] = sc.vel[a].ravel().copy()
    scenes.with_density_field(sc, "layers", rho0=1000.0, contrast=10.0)
    _run(gpu, sc, p)
    assert gpu.nRegions >= 1 and int(gpu.array("densityField")[0]) == 1
    vmax = max(np.abs(r).max() for r in ref)
    for a in range(3):
        ok = gpu.valid[a].ravel() > 0
        assert ok.sum() > 100
        assert np.abs(gpu.vel[a].ravel()[ok] - ref[a][ok]).max() <= 1e-6 * vmax

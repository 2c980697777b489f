"""Free-slip solids (ps_set_solid_boundary) on the GPU.

The oracle has no-slip walls only, so the checks here are physical (rigid sliding, a moving floor that does not drag), structural
against the no-slip path (which is checked against the oracle elsewhere), and the usual agreement of every solve route."""
import numpy as np
import pytest

from polystokes_amd import _abi as abi
from polystokes_amd import scenes

import children

pytestmark = pytest.mark.gpu
FREE, NO = abi.SOLID_FREE_SLIP, abi.SOLID_NO_SLIP


@pytest.fixture(scope="module")
def gpu():
    import polystokes_amd
    s = polystokes_amd.Solver(0)
    yield s
    s.close()


def _solver(mode=None):
    import polystokes_amd
    s = polystokes_amd.Solver(0)
    if mode is not None:
        assert s.set_solid_boundary(mode) == abi.SUCCESS
    return s


def _run(solver, sc, p):
    rc = solver.step(sc, p)
    assert rc == abi.SUCCESS, (rc, solver.last_error())
    return rc


def _scene(name):
    if name == "coil":
        return scenes.coil(32, tile=8)
    if name == "spheres":
        return scenes.spheres(32, tile=8)
    return scenes.blob()


def _liquid(s, a):
    """valid faces of the system (active or reduced): the faces inside a solid carry its collision velocity"""
    lab = s.array("face" + "XYZ"[a] + "Labels").reshape(s.valid[a].shape)
    return (s.valid[a] > 0) & ((lab == abi.ACTIVEFLUID) | (lab == abi.BOUNDARY) | (lab == abi.REDUCED))


def _tight(p, tol=1e-8):
    p.tolerance, p.maxSolverIterations = tol, 20000
    return p


# ---- 1, 2. physics ---------------------------------------------------------------------------------------------------------
def test_rigid_sliding_is_preserved():
    U = 1.0
    sc, p = scenes.sliding_block(32, U=U)
    _tight(p)
    free, no = _solver(FREE), _solver()
    try:
        _run(free, sc, p)
        _run(no, sc, p)
        assert free.nRegions > 0                                     # reduced tiles are in play
        assert int(free.array("solidBoundary")[0]) == FREE and int(no.array("solidBoundary")[0]) == NO
        assert int(free.array("solidSlipEdges")[0]) > 0
        for a, target in enumerate((U, 0.0, 0.0)):
            valid = _liquid(free, a)
            assert valid.any()
            assert np.abs(free.vel[a][valid] - target).max() <= 1e-6 * U, a
        # no-slip: the floor drags the faces next to it (the first liquid row of x faces, y in [2, 3) cells) by more than 10 %
        row = no.vel[0][:, 2, :][_liquid(no, 0)[:, 2, :]]
        assert row.size > 0 and row.min() <= 0.9 * U, row.min()
    finally:
        free.close()
        no.close()


def test_moving_floor_does_not_drag():
    V = 1.0
    sc, p = scenes.moving_floor(32, V=V)
    _tight(p)
    free, no = _solver(FREE), _solver(NO)
    try:
        _run(free, sc, p)
        _run(no, sc, p)
        for a in range(3):
            valid = _liquid(free, a)
            assert valid.any()
            assert np.abs(free.vel[a][valid]).max() <= 1e-6 * V, a
        drag = max(np.abs(no.vel[a][_liquid(no, a)]).max() for a in range(3))
        assert drag > 0.05 * V, drag
    finally:
        free.close()
        no.close()


# ---- 3. structure against no-slip ------------------------------------------------------------------------------------------
def _slip_columns(s):
    """reference system indices of the tau_e of the active edges a solid cuts (fluid weight < 1), from the arrays of the last setup"""
    dd = s.stats.dimData
    nP, nC = int(dd[12]), int(dd[0])
    nE = [int(dd[4]), int(dd[5]), int(dd[6])]
    cols = []
    off = nP + 3 * nC
    for ea, name in enumerate(("edgeYZ", "edgeXZ", "edgeXY")):
        lab = s.array(name + "Labels")
        act = (lab == abi.ACTIVEFLUID) | (lab == abi.BOUNDARY)
        cut = act & (s.array(name + "FluidWeights") < 1.0)
        idx = s.array(name + "ActiveIndices")
        assert np.all(idx[act] >= 0) and np.all(idx[act] < nE[ea])
        cols.append(off + idx[cut].astype(np.int64))
        off += nE[ea]
    return np.concatenate(cols)


def _drop_columns(M, cols):
    M = M.tocsc(copy=True)
    keep = np.ones(M.shape[1], bool)
    keep[cols] = False
    M = M @ __import__("scipy.sparse", fromlist=["diags"]).diags(keep.astype(np.float64))
    M = M.tocsr()
    M.eliminate_zeros()
    M.sort_indices()
    return M


def _csr_equal(A, B):
    A, B = A.tocsr(), B.tocsr()
    A.sort_indices()
    B.sort_indices()
    return A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and np.array_equal(A.data, B.data)


_FIELDS = [s + k for s in abi.SAMPLE_NAMES for k in ("Labels", "ActiveIndices", "ReducedIndices", "LiquidWeights", "FluidWeights")]


@pytest.mark.parametrize("name", ["coil", "spheres", "blob"])
def test_structure_against_no_slip(name):
    sc, p = _scene(name)
    free, no = _solver(FREE), _solver()
    try:
        for s in (free, no):
            s.upload(sc, p)
            assert s.setup() == abi.SUCCESS
        assert list(free.stats.dimData) == list(no.stats.dimData)
        for f in _FIELDS + ["faceRowX", "faceRowY", "faceRowZ", "sysPerm", "rowPerm"]:
            assert np.array_equal(free.array(f), no.array(f)), f
        cols = _slip_columns(no)
        assert np.array_equal(np.sort(cols), np.sort(_slip_columns(free)))
        assert cols.size > 0
        assert int(free.array("solidSlipEdges")[0]) == cols.size
        with pytest.raises(KeyError):
            no.array("solidSlipEdges")
        S0, St0 = no.S_matrices()
        S1, St1 = free.S_matrices()
        # the dropped columns held entries under no-slip: the edges really were coupled
        assert np.diff(St0.indptr)[cols].sum() > 0
        # the pattern is no-slip's (the dropped entries are explicit zeros), every other value is bit for bit no-slip's
        for A1, A0 in ((S1, S0), (St1, St0)):
            assert np.array_equal(A1.indptr, A0.indptr) and np.array_equal(A1.indices, A0.indices)
        zero = np.isin(S1.indices, cols)
        assert np.all(S1.data[zero] == 0) and np.array_equal(S1.data[~zero], S0.data[~zero])
        assert np.all(S0.data[zero] != 0)
        # without the explicit zeros: no-slip with exactly the tau columns / rows of the cut edges removed
        S1z, St1z = S1.copy(), St1.copy()
        S1z.eliminate_zeros()
        St1z.eliminate_zeros()
        assert _csr_equal(S1z, _drop_columns(S0, cols))
        assert _csr_equal(St1z, _drop_columns(St0.T, cols).T)
        # rhs: 0 on the dropped edges, bit for bit the same everywhere else
        nP = no.nP
        r0, r1 = no.array("stressRHSVector"), free.array("stressRHSVector")
        drop = np.zeros(r0.size, bool)
        drop[cols - nP] = True
        assert np.all(r1[drop] == 0) and np.array_equal(r1[~drop], r0[~drop])
        assert np.array_equal(free.array("pressureRHSVector"), no.array("pressureRHSVector"))
        assert np.array_equal(free.array("uInv"), no.array("uInv"))
        assert np.array_equal(free.array("McInv"), no.array("McInv"))
        assert np.array_equal(free.array("activeRHSVector"), no.array("activeRHSVector"))
    finally:
        free.close()
        no.close()


# ---- 4. a well-posed system ------------------------------------------------------------------------------------------------
# The stop rule bounds the residual, not the error: on the stiff spheres scene the preconditioners' solutions lie 1e-4 (identity) and
# 3.5e-7 (Chebyshev) apart in norm under no-slip at tolerance 1e-8, and slab / brick velocities 9e-5 from the single domain's.  Free slip
# is held to max(10 tol, 2x what no-slip shows in the same run).
def _bound(tol, no_slip_err):
    return max(10 * tol, 2 * no_slip_err)


def test_well_posed_and_preconditioners_agree():
    sc, p = scenes.spheres(32, tile=8)
    assert any(np.abs(v).max() > 0 for v in sc.collisionvel)        # moving solids
    _tight(p)
    pres = (abi.PRE_IDENTITY, abi.PRE_DIAGONAL, abi.PRE_CHEBYSHEV, abi.PRE_CHEBYSHEV_F32)
    err = {}
    for mode in (NO, FREE):
        s = _solver(mode)
        try:
            xs = {}
            for pre in pres:
                p.preconditioner = pre
                _run(s, sc, p)
                xs[pre] = s.array("solutionVector")
            ref = xs[abi.PRE_DIAGONAL]
            err[mode] = {pre: np.linalg.norm(xs[pre] - ref) / np.linalg.norm(ref) for pre in pres}
            if mode == FREE:
                S, St = s.S_matrices()
                assert _csr_equal(S.T, St)
                rng = np.random.RandomState(7)
                n = s.nP + s.nT
                for _ in range(3):
                    x, y = rng.standard_normal(n), rng.standard_normal(n)
                    Ax, Ay = s.apply(x), s.apply(y)
                    assert abs(x @ Ay - y @ Ax) <= 1e-10 * np.sqrt(abs(x @ Ax) * abs(y @ Ay))
                    assert x @ Ax < 0 and y @ Ay < 0                   # definite (A is negative definite in this sign convention)
        finally:
            s.close()
    for pre in pres:
        assert err[FREE][pre] <= _bound(p.tolerance, err[NO][pre]), (pre, err)


_CHILD = ("sc, p = scenes.spheres(32, tile=8)\n"
          "p.preconditioner = {pre}\np.tolerance = 1e-8\np.maxSolverIterations = 20000\n"
          "s = polystokes_amd.Solver(0)\ns.set_solid_boundary(abi.SOLID_FREE_SLIP)\nrc = s.step(sc, p)\n"
          "np.save({out!r}, s.array('solutionVector'))\n"
          "print('RESULT ' + json.dumps(dict(rc=rc, coded=int(s.array('valuesCoded')[0]), c16=int(s.array('columns16')[0]),"
          " slip=int(s.array('solidSlipEdges')[0]))))\n")


def _child(tmp_path, tag, env, pre):
    out = str(tmp_path / (tag + ".npy"))
    info = children.run_python(_CHILD.format(pre=pre, out=out), limit=300, env=env).result()
    assert info["rc"] == abi.SUCCESS, (tag, info)
    return info, np.load(out)


def test_storage_fallbacks_agree(tmp_path):
    """the fp64-value stream, the 32-bit CSR kernels and the 4-entries-per-lane kernels hold the empty edge columns as well"""
    for pre in (abi.PRE_DIAGONAL, abi.PRE_CHEBYSHEV_F32):
        base, x = _child(tmp_path, f"base{pre}", {}, pre)
        assert base["coded"] == 1 and base["slip"] > 0
        for tag, env in (("fp64", {"PS_FORCE_FP64_VALUES": "1"}), ("col32", {"PS_COL32": "1"}), ("noell", {"PS_NO_ELL": "1"})):
            info, y = _child(tmp_path, f"{tag}{pre}", env, pre)
            assert info["slip"] == base["slip"]
            if tag == "fp64":
                assert info["coded"] == 0
            if tag == "col32":
                assert info["c16"] == 0
            assert np.linalg.norm(y - x) <= 10 * 1e-8 * np.linalg.norm(x), (tag, pre, np.linalg.norm(y - x) / np.linalg.norm(x))


# ---- 5. decompositions -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [None, (2, 2, 2)])
def test_decompositions_match_single_domain(dims):
    import polystokes_amd
    world = 2 if dims is None else 8
    sc, p = scenes.spheres(32, tile=8)
    _tight(p)
    err = {}
    for mode in (NO, FREE):
        single = _solver(mode)
        grp = polystokes_amd.Group(world, dims=dims)
        try:
            assert grp.set_solid_boundary(mode) == abi.SUCCESS
            _run(single, sc, p)
            assert grp.solve_scene(sc, p) == abi.SUCCESS
            for r in grp.ranks:
                assert int(r.array("solidBoundary")[0]) == mode
            if mode == FREE:
                assert sum(int(r.array("solidSlipEdges")[0]) for r in grp.ranks) >= int(single.array("solidSlipEdges")[0]) > 0
            for a in range(3):
                assert np.array_equal(grp.valid[a], single.valid[a])
            err[mode] = max(np.abs(grp.vel[a] - single.vel[a]).max() / max(np.abs(single.vel[a]).max(), 1e-30) for a in range(3))
        finally:
            grp.close()
            single.close()
    assert err[FREE] <= _bound(p.tolerance, err[NO]), err


# ---- 6. combined with other features ---------------------------------------------------------------------------------------
def test_exported_system_solves_the_same(gpu, tmp_path):
    import scipy.io
    sc, p = scenes.coil(32, tile=8)
    _tight(p)
    p.preconditioner = abi.PRE_DIAGONAL
    gpu.set_solid_boundary(FREE)
    try:
        _run(gpu, sc, p)
        pre = str(tmp_path) + "/slip."
        gpu.export_component_matrices(pre)
        x_mem = np.asarray(scipy.io.mmread(pre + "solutionVector.mtx")).ravel()
        rc, x = gpu.solve_exported_system(pre, p, sc.dt, x_mem.size)
        assert rc == abi.SUCCESS
        assert np.linalg.norm(x - x_mem) <= 10 * p.tolerance * np.linalg.norm(x_mem)
    finally:
        gpu.set_solid_boundary(NO)


def test_with_warm_start_density_field_and_surface_tension():
    sc, p = scenes.sliding_block(32)
    scenes.with_density_field(sc, "layers")
    sc.surface_tension = 0.5
    _tight(p, 1e-7)
    p.preconditioner = abi.PRE_CHEBYSHEV_F32
    s = _solver(FREE)
    try:
        s.set_warm_start(abi.WARM_PREVIOUS_STEP)
        for step in range(2):
            s.upload(sc, p)
            assert s.step_device() == abi.SUCCESS, s.last_error()
            s.download()
            assert int(s.array("densityField")[0]) == 1 and float(s.array("surfaceTension")[0]) == 0.5
            assert int(s.array("solidBoundary")[0]) == FREE and int(s.array("solidSlipEdges")[0]) > 0
            for a in range(3):
                assert np.isfinite(s.vel[a]).all()
        assert int(s.array("warmStartUsed")[0]) == 1
    finally:
        s.close()


# ---- 7. off means off ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["coil", "spheres"])
def test_no_slip_is_the_default_path(name):
    sc, p = _scene(name)
    a, b = _solver(), _solver(FREE)
    try:
        assert b.set_solid_boundary(NO) == abi.SUCCESS
        _run(a, sc, p)
        _run(b, sc, p)
        for q in range(3):
            assert a.vel[q].tobytes() == b.vel[q].tobytes() and a.valid[q].tobytes() == b.valid[q].tobytes()
        assert a.array("solutionVector").tobytes() == b.array("solutionVector").tobytes()
        assert int(a.array("solidBoundary")[0]) == NO and int(b.array("solidBoundary")[0]) == NO
    finally:
        a.close()
        b.close()


def test_bad_mode_keeps_the_setting():
    sc, p = scenes.moving_floor(32)
    s = _solver(FREE)
    try:
        for bad in (2, -1, 99):
            assert s.set_solid_boundary(bad) == abi.INVALID
            assert "ps_set_solid_boundary" in s.last_error()
        s.upload(sc, p)
        assert s.setup() == abi.SUCCESS
        assert int(s.array("solidBoundary")[0]) == FREE and int(s.array("solidSlipEdges")[0]) > 0
        # the setting persists across uploads until changed
        assert s.set_solid_boundary(NO) == abi.SUCCESS
        s.upload(sc, p)
        assert s.setup() == abi.SUCCESS
        assert int(s.array("solidBoundary")[0]) == NO
    finally:
        s.close()

"""Velocity recovery and write-back restated in numpy, fp64 throughout, on a GIVEN solution vector x.

    active faces    u   = dt McInv (rhs_a / dt - C x),             C = [G Dt]                         (Solver.cpp:492-510)
    reduced regions v_r = BInv_r (rhs_r / dt - [JG JDt]_r x),      velocity C_f . v_r at every face whose ReducedIndices is >= 0
    write-back      applySolutionToVelocity                                                         (Solver.cpp:937-1028)

Two solves that both meet the stop rule differ by per cents in u on the stiff scenes (the recovery differences 1e5-sized terms: "AMP",
DESIGN.md section 4), so the velocity tests that compare two solves carry bounds of 2 % and more.  Same x and same blocks give the same u
up to the rounding of the sums: this module computes u from the solve's own x, and a running error bound E_f of every face next to it.

    |vel - u_ref64| <= ulp32(|u_ref64| + E_f) / 2 + E_f                                                 (check)

E_f is the expression evaluated on absolute values, every partial result weighted by (summed terms + rounded factors) 2^-53 up to
that point.  No measured constant enters.  Faces that keep the input, take the collision velocity or take 0 are compared bit for bit.

Block sources: from_oracle(o, scene) and from_solver(solver, scene).  A decomposition's merged x is computed on the blocks of a
single-domain setup of the same scene."""
import copy

import numpy as np
import scipy.sparse as sp

from polystokes_amd import _abi as abi

from helpers import basis_rows, per_row

RD = abi.REDUCED_DOF
U64 = 2.0 ** -53
# roundings of one basis entry C_f[m] before it is used: the offset (index * dx - com: two) and a monomial of up to three factors and a
# constant (-2 x z, -0.5 z z: three)
BASIS_ROUNDINGS = 5

KEEP, REDUCED, ACTIVE, SOLID, ZERO = 0, 1, 2, 3, 4
CATEGORY_NAMES = {KEEP: "untouched", REDUCED: "reduced", ACTIVE: "active", SOLID: "solid", ZERO: "zero"}


class Blocks:
    """What recovery and write-back read.  C: (nA, n) CSR [G Dt].  J: (26 R, n) CSR [JG JDt]; Jabs / Jterms: the sum of the absolute
    values of the products that form an entry of J x, and how many there are (from_solver: the device forms J^T (S_r x) row by row, a sum
    at least as large and as long as |J| |x|).  Face arrays: flat, x fastest, one per axis."""

    def __init__(self, scene, C, J, Jabs, Jterms, McInv, rhsA, rhsR, BInv, COM, labels, act, red, face_rows):
        self.scene, self.dx, self.dt = scene, float(scene.dx), float(scene.dt)
        self.C, self.J, self.Jabs, self.Jterms = C.tocsr(), J.tocsr(), Jabs.tocsr(), np.asarray(Jterms, np.float64)
        self.McInv, self.rhsA, self.rhsR = (np.asarray(v, np.float64) for v in (McInv, rhsA, rhsR))
        self.R = len(self.rhsR) // RD
        self.BInv = np.asarray(BInv, np.float64).reshape(self.R, RD, RD)
        self.COM = np.asarray(COM, np.float64).reshape(self.R, 3)
        self.labels, self.act, self.red = labels, act, red
        self.face_rows = face_rows                     # per axis: the active row of every face (-1: none), reference numbering
        self.nA = len(self.McInv)


def _face_state(src, nA):
    labels = [src.array("face" + a + "Labels") for a in "XYZ"]
    act = [src.array("face" + a + "ActiveIndices") for a in "XYZ"]
    red = [src.array("face" + a + "ReducedIndices") for a in "XYZ"]
    # the row of every active face: per_row scatters a per-face quantity into row order (axis-local and global numbering both), so the
    # global face number scattered that way is the face of every row
    sizes = [len(v) for v in act]
    base = np.concatenate([[0], np.cumsum(sizes)])
    face_of_row = per_row(src, [np.arange(sizes[a], dtype=np.float64) + base[a] for a in range(3)]).astype(np.int64)
    row_of_face = np.full(base[3], -1, np.int64)
    row_of_face[face_of_row] = np.arange(nA)
    rows = [row_of_face[base[a]:base[a + 1]] for a in range(3)]
    for a in range(3):
        assert np.array_equal(rows[a] >= 0, act[a] >= 0)
    return labels, act, red, rows


def from_oracle(o, scene):
    """the oracle's blocks (o.csr, o.array) after o.run(scene, params)"""
    nA = o.nA
    C = sp.hstack([o.csr("G"), o.csr("Dt")]).tocsr() if nA else sp.csr_matrix((0, o.nP + o.nT))
    J = sp.hstack([o.csr("JG"), o.csr("JDt")]).tocsr()
    Jabs = abs(J)
    Jterms = np.diff(Jabs.indptr)
    labels, act, red, rows = _face_state(o, nA)
    return Blocks(scene, C, J, Jabs, Jterms, o.array("McInv"), o.array("activeRHSVector"), o.array("reducedRHSVector"),
                  o.array("Inv_Mr_plus_2JDtuDJ"), o.array("reducedRegionCOM"), labels, act, red, rows)


def from_solver(solver, scene):
    """the device's blocks after setup() or a step: S_matrices() with the on-the-fly basis (what helpers.materialise_blocks forms), McInv,
    the right-hand sides, BInv, the centres of mass and the face Labels / ActiveIndices / ReducedIndices"""
    nA, R = solver.nA, solver.nRegions
    S, _ = solver.S_matrices()
    C = S[:nA, :].tocsr()
    Sr = S[nA:, :].tocsr()
    nRr = Sr.shape[0]
    assert nRr == len(solver.array("reducedRowFace"))
    if nRr and R:
        packed, reg = solver.array("reducedRowFace"), solver.array("reducedRowRegion")
        i, j, k, a = packed & 1023, (packed >> 10) & 1023, (packed >> 20) & 1023, packed >> 30
        pos = np.stack([i, j, k], axis=1).astype(np.float64)
        pos[np.arange(nRr), a] -= 0.5
        com = solver.array("reducedRegionCOM").reshape(-1, 3)
        Cm = basis_rows(pos * scene.dx - com[reg], a)
        rws = (reg[:, None] * RD + np.arange(RD)[None, :]).ravel()
        cls = np.repeat(np.arange(nRr), RD)
        Jb = sp.csr_matrix((Cm.ravel(), (rws, cls)), shape=(R * RD, nRr))
        Jb.eliminate_zeros()
        J = (Jb @ Sr).tocsr()
        # |J^T| |S_r| and the number of products behind every entry of J x, as the device sums them (k_tile_gather / k_tile_apply)
        Jabs = (abs(Jb) @ abs(Sr)).tocsr()
        Jterms = np.asarray((Jb != 0).astype(np.float64) @ np.diff(Sr.indptr).astype(np.float64)).ravel()
    else:
        J = sp.csr_matrix((R * RD, S.shape[1]))
        Jabs, Jterms = J, np.zeros(R * RD)
    labels, act, red, rows = _face_state(solver, nA)
    return Blocks(scene, C, J, Jabs, Jterms, solver.array("McInv"), solver.array("activeRHSVector"), solver.array("reducedRHSVector"),
                  solver.array("Inv_Mr_plus_2JDtuDJ"), solver.array("reducedRegionCOM"), labels, act, red, rows)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
def recover(b, x, flip_region=None):
    """recoverVelocityFromPressureStress on x with the running error bounds: (u (nA), E_u, the active expression on absolute values,
    v (R, 26), E_v, the reduced expression on absolute values).  flip_region: a region whose rhs_r / dt - w becomes rhs_r / dt + w (a
    mutant for the self-checks)."""
    x = np.asarray(x, np.float64)
    ax = np.abs(x)
    dt, inv_dt = b.dt, 1.0 / b.dt
    # active: dt McInv (rhs / dt - C x).  Terms: the row's products and the right-hand side; factors: 1 / dt, rhs / dt, McInv, dt
    s = b.C @ x
    u = dt * b.McInv * (inv_dt * b.rhsA - s)
    absu = dt * np.abs(b.McInv) * (np.abs(b.rhsA) * inv_dt + abs(b.C) @ ax)
    Eu = absu * (np.diff(b.C.indptr) + 1 + 4) * U64
    # reduced: w = J x (the gather), t = rhs_r / dt - w, v = BInv t (the 26 x 26 product)
    w = b.J @ x
    t = inv_dt * b.rhsR - w
    if flip_region is not None:
        t[flip_region * RD:(flip_region + 1) * RD] = (inv_dt * b.rhsR + w)[flip_region * RD:(flip_region + 1) * RD]
    T = np.abs(b.rhsR) * inv_dt + b.Jabs @ ax
    kT = b.Jterms + BASIS_ROUNDINGS + 1 + 2            # the gather's products with their basis entry, the right-hand side, 1 / dt and rhs / dt
    v = np.einsum("rmn,rn->rm", b.BInv, t.reshape(b.R, RD))
    aB = np.abs(b.BInv)
    V = np.einsum("rmn,rn->rm", aB, T.reshape(b.R, RD))
    Ev = np.einsum("rmn,rn->rm", aB, (T * (kT + RD)).reshape(b.R, RD)) * U64
    return u, Eu, absu, v, Ev, V


def reduced_basis(b, axis, flat_idx, regions, half_cell=True):
    """C_f of the faces flat_idx of an axis about their regions' centres of mass: the offset takes the -1/2 cell along the face's own axis"""
    sh = abi.grid_shapes(b.scene.nx, b.scene.ny, b.scene.nz)["face" + "XYZ"[axis]]
    k, j, i = np.unravel_index(flat_idx, sh)
    pos = np.stack([i, j, k], axis=1).astype(np.float64)
    if half_cell:
        pos[:, axis] -= 0.5
    return basis_rows(pos * b.dx - b.COM[regions], np.full(len(flat_idx), axis))


def categories(b, axis):
    """the branch of applySolutionToVelocity every face of an axis takes"""
    lab, act, red = b.labels[axis], b.act[axis], b.red[axis]
    cat = np.full(len(lab), ZERO, np.int8)
    cat[lab == abi.SOLID] = SOLID
    cat[act >= 0] = ACTIVE
    cat[red >= 0] = REDUCED
    cat[(lab == abi.UNSOLVED) | (lab == abi.UNASSIGNED)] = KEEP
    return cat


def velocity(b, x, apply=True, half_cell=True, keep=None, flip_region=None):
    """Write-back of x on the blocks b: per axis (vel fp32, u_ref64, E_f, category, |expression| on absolute values), flat arrays.
    apply = False: a step whose results are dropped (every face keeps the input).  keep: per axis a mask of faces that keep the input
    whatever their label (a rank's faces owned by another rank)."""
    u, Eu, absu, v, Ev, V = recover(b, x, flip_region)
    out = []
    for a in range(3):
        vin = np.asarray(b.scene.vel[a], np.float32).ravel()
        cvel = np.asarray(b.scene.collisionvel[a], np.float32).ravel()
        cat = categories(b, a)
        if not apply:
            cat[:] = KEEP
        if keep is not None:
            cat[keep[a]] = KEEP
        ref = np.zeros(len(vin))
        E = np.zeros(len(vin))
        mag = np.zeros(len(vin))
        m = cat == KEEP
        ref[m] = vin[m]
        m = cat == SOLID
        ref[m] = cvel[m]
        m = cat == ACTIVE
        rows = b.face_rows[a][m]
        ref[m], E[m] = u[rows], Eu[rows]
        mag[m] = absu[rows]
        idx = np.nonzero(cat == REDUCED)[0]
        if len(idx):
            r = b.red[a][idx]
            Cf = reduced_basis(b, a, idx, r, half_cell)
            aC = np.abs(Cf)
            ref[idx] = np.einsum("fm,fm->f", Cf, v[r])
            # the 26-term dot: v carries E_v, every product its basis entry's roundings and the sum's 26
            E[idx] = np.einsum("fm,fm->f", aC, Ev[r] + (RD + BASIS_ROUNDINGS) * U64 * V[r])
            mag[idx] = np.einsum("fm,fm->f", aC, V[r])
        out.append((ref.astype(np.float32), ref, E, cat, mag))
    return out


def ulp32(y):
    """the spacing of fp32 at |y| (y fp64): 2^(e - 23), 2^-149 below the normal range"""
    y = np.abs(np.asarray(y, np.float64))
    _, e = np.frexp(y)
    e = np.where(y >= 2.0 ** -126, e - 1, -126)
    return np.ldexp(1.0, e - 23)


def bits(v):
    return np.ascontiguousarray(v, np.float32).view(np.uint32)


def compare(ref, vel):
    """Every face of the three axes against the reference (the output of velocity()).  Returns a dict: 'bad' (the first faces outside the
    bound, as (axis, face, category, got, ref, bound)), 'nbad' (faces outside the bound per category name), 'counts' per category,
    'ratio' (largest |d| / bound over the computed faces: 1 is reached by the fp32 rounding alone), 'e_used' (largest share of E_f a
    face needs beyond the fp32 rounding of the reference: 0 where the device has the reference's bits), 'cancel' (largest expression on
    absolute values / |u|)."""
    bad, counts, nbad = [], {c: 0 for c in CATEGORY_NAMES}, {n: 0 for n in CATEGORY_NAMES.values()}
    ratio = e_used = cancel = 0.0
    for a in range(3):
        _, r64, E, cat, mag = ref[a]
        got = np.asarray(vel[a], np.float32).ravel()
        assert got.shape == r64.shape, (a, got.shape, r64.shape)
        comp = (cat == ACTIVE) | (cat == REDUCED)
        d = np.abs(got.astype(np.float64) - r64)
        bound = 0.5 * ulp32(np.abs(r64) + E) + E
        wrong = np.where(comp, ~(d <= bound), bits(got) != bits(r64.astype(np.float32)))     # (~(<=): a NaN is outside)
        for c in counts:
            counts[c] += int((cat == c).sum())
            nbad[CATEGORY_NAMES[c]] += int((wrong & (cat == c)).sum())
        for c in counts:
            for f in np.nonzero(wrong & (cat == c))[0][:3]:
                bad.append((a, int(f), CATEGORY_NAMES[c], float(got[f]), float(r64[f]), float(bound[f])))
        if comp.any():
            ratio = max(ratio, float((d[comp] / bound[comp]).max()))
            over = np.maximum(d - 0.5 * ulp32(r64), 0.0)[comp]
            Ec = E[comp]
            if (Ec > 0).any():
                e_used = max(e_used, float((over[Ec > 0] / Ec[Ec > 0]).max()))
            nz = comp & (np.abs(r64) > 0)
            if nz.any():
                cancel = max(cancel, float((mag[nz] / np.abs(r64[nz])).max()))
    return {"bad": bad, "nbad": nbad, "counts": counts, "ratio": ratio, "e_used": e_used, "cancel": cancel}


def solid_moving(b):
    """faces that take a non-zero collision velocity"""
    return sum(int(((categories(b, a) == SOLID) & (np.asarray(b.scene.collisionvel[a]).ravel() != 0)).sum()) for a in range(3))


def check(b, x, vel, need=(), apply=True, keep=None):
    """assert the bound on every face and that the categories in `need` ('active', 'reduced', 'solid_moving', 'untouched') are non-empty;
    returns compare()'s dict"""
    res = compare(velocity(b, x, apply=apply, keep=keep), vel)
    assert not res["bad"], (res["nbad"], res["bad"][:12])
    have = {"active": res["counts"][ACTIVE], "reduced": res["counts"][REDUCED], "untouched": res["counts"][KEEP],
            "solid_moving": solid_moving(b) if apply else 0}
    for c in need:
        assert have[c] > 0, (c, have)
    res["have"] = have
    return res


# ---- a rank of a decomposition ---------------------------------------------------------------------------------------------------------------
def halo_faces(act, face_row, red, labels):
    """per axis: the active faces of a rank whose row another rank owns (k_writeback leaves them untouched)"""
    return [(act[a] >= 0) & (face_row[a] < 0) & (red[a] < 0) & (labels[a] != abi.UNSOLVED) & (labels[a] != abi.UNASSIGNED) for a in range(3)]


def check_halo_kept(vin, vout, halo, ref32=None):
    """a rank's output holds the input, bit for bit, on its halo faces.  Returns (halo faces, those among them whose recovered velocity
    ref32 differs from the input: only there would an overwritten face show)"""
    n = visible = 0
    for a in range(3):
        m = np.asarray(halo[a]).ravel()
        wrong = m & (bits(np.asarray(vout[a]).ravel()) != bits(np.asarray(vin[a]).ravel()))
        assert not wrong.any(), (a, int(wrong.sum()), np.nonzero(wrong)[0][:5].tolist())
        n += int(m.sum())
        if ref32 is not None:
            visible += int((m & (bits(np.asarray(ref32[a]).ravel()) != bits(np.asarray(vin[a]).ravel()))).sum())
    return n, visible


# ---- the small single-domain scenes and what each is there for -----------------------------------------------------------------------------
def small_scenes():
    """the twelve scenes of test_gpu_parity, spheres(32, tile=8) and coil(32, tile=8): name -> () -> (scene, params)"""
    import test_gpu_parity
    from polystokes_amd import scenes
    out = dict(test_gpu_parity.SCENES)
    out["spheres32_t8"] = lambda: scenes.spheres(32, tile=8)
    out["coil32_t8"] = lambda: scenes.coil(32, tile=8)
    return out


_ALL = ("active", "reduced", "solid_moving", "untouched")
# The face categories a scene counts for: they are non-empty in it, and every mutant of the matching kind breaks the bound in it
# (test_recovery_ref_cpu.py).  The cavities' McInv = 1 / (rho dx^3) is a power of two times a short fraction that fp32 holds exactly: the
# fp32-McInv mutant survives there, so they do not count for the active faces.  The droplet at rest has x = 0 and right-hand sides 0.
CLAIMS = {
    "cavity32": ("reduced",), "cavity20_t10_p1": ("reduced",), "cavity33_linear": ("reduced",),
    "beam32_uniform": ("active", "untouched"),
    "coil48": ("active", "reduced", "untouched"), "coil32_t8": ("active", "reduced", "untouched"),
    "blob0": _ALL, "blob1_t7": _ALL, "blob2_notile": _ALL, "blob3_L3S3": _ALL, "blob4_L1S0": _ALL,
    "spheres40": _ALL, "spheres32_t8": _ALL,
    "droplet24": ("untouched",),
}
X_KINDS = ("converged", "five_iterations", "no_solve")


def with_x_kind(p, kind):
    """params of the three kinds of x: a converged solve, the unconverged iterate of maxSolverIterations = 5 that is kept, a doSolve = 0 step
    (x = 0: it counts for no computed category)"""
    if kind == "five_iterations":
        p.maxSolverIterations, p.keepNonConvergedResults = 5, 1
    elif kind == "no_solve":
        p.doSolve, p.keepNonConvergedResults = 0, 1
    else:
        assert kind == "converged", kind
    return p


def claims(name, kind):
    c = CLAIMS[name]
    return tuple(q for q in c if q in ("solid_moving", "untouched")) if kind == "no_solve" else c


# ---- mutants of the restatement: each must leave the bound (test_recovery_ref_cpu.py) ------------------------------------------------------
def mutant_x_fp32(b, x):
    return b, np.asarray(x, np.float32).astype(np.float64), {}


def mutant_drop_entry(b, x):
    """the entry of the middle active row with the smallest non-zero product is dropped"""
    m = copy.copy(b)
    C = b.C.copy()
    x = np.asarray(x, np.float64)
    live = np.nonzero(np.asarray(abs(C) @ np.abs(x)).ravel() > 0)[0]          # rows with a non-zero product
    assert len(live), "no active row has a non-zero product: nothing to drop"
    f = int(live[np.searchsorted(live, b.nA // 2) % len(live)])             # the first such row from the middle on (else from the start)
    sl = slice(C.indptr[f], C.indptr[f + 1])
    prod = np.abs(C.data[sl] * x[C.indices[sl]])
    prod[prod == 0] = np.inf
    C.data[C.indptr[f] + int(np.argmin(prod))] = 0.0
    m.C = C
    return m, x, {}


def mutant_mcinv_fp32(b, x):
    m = copy.copy(b)
    m.McInv = b.McInv.astype(np.float32).astype(np.float64)
    return m, x, {}


def mutant_no_half_cell(b, x):
    return b, x, {"half_cell": False}


def mutant_flip_sign(b, x):
    return b, x, {"flip_region": b.R // 2}


# mutant -> the category whose faces it must push outside the bound
MUTANTS = {"x_fp32": (mutant_x_fp32, "active"), "x_fp32_reduced": (mutant_x_fp32, "reduced"), "drop_entry": (mutant_drop_entry, "active"),
           "mcinv_fp32": (mutant_mcinv_fp32, "active"), "no_half_cell": (mutant_no_half_cell, "reduced"),
           "flip_sign": (mutant_flip_sign, "reduced")}

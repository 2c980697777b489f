"""The velocity-recovery restatement (recovery_ref.py) checks itself on the CPU before the GPU tests rely on it.

1. Against the oracle: fed the oracle's own x and blocks it must meet its own bound against the oracle's velX/Y/Z on every face (it
   reproduces them bit for bit on most scenes) for three kinds of x: a converged solve, the kept iterate of maxSolverIterations = 5 and a
   doSolve = 0 step.
2. Mutants of the restatement must leave the bound on at least one face of the matching category in every case that counts for it
   (recovery_ref.CLAIMS): x rounded to fp32, one entry of one active row dropped, McInv rounded to fp32, the reduced basis without the
   -1/2 cell, rhs_r / dt + w in one region, and one halo face of a rank overwritten."""
import numpy as np
import pytest

import recovery_ref as rr

SCENES = rr.small_scenes()
_cache = {}


def _case(oracle_mod, name, kind):
    key = (name, kind)
    if key not in _cache:
        _cache.clear()                                    # (one case in memory at a time: the parametrisation runs case by case)
        sc, p = SCENES[name]()
        rr.with_x_kind(p, kind)
        o = oracle_mod.Oracle()
        o.run(sc, p)
        x = o.array("solutionVector")
        assert len(x) == o.nP + o.nT
        _cache[key] = (sc, p, o, rr.from_oracle(o, sc), x, [o.array("vel" + a) for a in "XYZ"])
    return _cache[key]


CASES = [(n, k) for n in SCENES for k in rr.X_KINDS]


@pytest.mark.parametrize("name,kind", CASES)
def test_restatement_meets_its_bound_against_the_oracle(oracle_mod, name, kind):
    sc, p, o, b, x, vel = _case(oracle_mod, name, kind)
    if kind == "no_solve":
        assert not np.any(x)
    elif name != "droplet24":
        assert np.any(x)
    res = rr.check(b, x, vel, need=rr.claims(name, kind))
    # write-back follows the labels; the oracle follows its valid faces: the same faces
    for a in range(3):
        assert np.array_equal(o.array("valid" + "XYZ"[a]) == 0, rr.categories(b, a) == rr.KEEP)
    assert res["ratio"] <= 1.0


MUTANT_CASES = [(n, k, m) for n in SCENES for k in rr.X_KINDS[:2] for m, (_, cat) in rr.MUTANTS.items() if cat in rr.claims(n, k)]


@pytest.mark.parametrize("name,kind,mutant", MUTANT_CASES)
def test_mutants_leave_the_bound(oracle_mod, name, kind, mutant):
    sc, p, o, b, x, vel = _case(oracle_mod, name, kind)
    fn, cat = rr.MUTANTS[mutant]
    mb, mx, kw = fn(b, x)
    res = rr.compare(rr.velocity(mb, mx, **kw), vel)
    assert res["nbad"][cat] > 0, (name, kind, mutant, res["nbad"])


@pytest.mark.parametrize("name", ["blob0", "spheres32_t8", "coil32_t8"])
def test_an_overwritten_halo_face_is_seen(oracle_mod, name):
    """a rank made up from the single domain: the upper half of the grid belongs to 'another rank' (its active faces have no row here)"""
    sc, p, o, b, x, vel = _case(oracle_mod, name, "converged")
    ref = rr.velocity(b, x)
    face_row = []
    for a in range(3):
        rows = b.face_rows[a].copy()
        rows[len(rows) // 2:] = -1
        face_row.append(rows)
    halo = rr.halo_faces(b.act, face_row, b.red, b.labels)
    vin = [np.asarray(sc.vel[a]).ravel() for a in range(3)]
    out = [np.where(halo[a], vin[a], ref[a][0]) for a in range(3)]
    ref32 = [ref[a][0] for a in range(3)]
    n, visible = rr.check_halo_kept(vin, out, halo, ref32)
    assert n > 0 and 2 * visible >= n, (n, visible)       # (a face whose recovered velocity has the input's bits cannot show an overwrite)
    for a in range(3):
        f = np.nonzero(halo[a] & (rr.bits(ref32[a]) != rr.bits(vin[a])))[0]
        mutant = [v.copy() for v in out]
        mutant[a][f[len(f) // 2]] = ref32[a][f[len(f) // 2]]   # the mutant: one halo face takes the recovered velocity
        with pytest.raises(AssertionError):
            rr.check_halo_kept(vin, mutant, halo)

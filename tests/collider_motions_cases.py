"""Inputs shared by the collider-motion tests (test_collider_motions_ref_cpu.py, test_gpu_collider_motions.py), and the child process of the
poisoned-buffer test:  python collider_motions_cases.py paint <case>  prints digests of what a paint and the step after it leave.

Grids whose extents differ and are no multiples of 64 along x (a swapped axis or a wave tail shows); id fields None, mod3 and spheres of
collider_loads_cases.py (the last holds id 8 outside a count of 8) and mod67 for a count of 64; crafted SDFs with D_U == D_L, with NaN
cells, and with negateCollision = 0; tables with pure translation, pure rotation about a point off the grid, both; a non-zero orig."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from polystokes_amd import _abi as abi  # noqa: E402
from polystokes_amd import scenes  # noqa: E402

import collider_loads_cases as loads_cases  # noqa: E402
import collider_motions_ref as ref  # noqa: E402

ARRAYS = ("colliderMotions", "colliderMotionTable", "colliderMotionFaces", "collisionVelocityX", "collisionVelocityY", "collisionVelocityZ")
GRID_ARRAYS = ARRAYS[3:]


def box(kind="random", seed=3):
    """A 20 x 12 x 9 box of random SDF values with a random collisionvel: nothing here is meant to be stepped.  'ties': the values are
    multiples of 0.5, so most neighbours tie; 'nan': a few cells hold NaN."""
    nx, ny, nz = 20, 12, 9
    rng = np.random.RandomState(seed)
    col = rng.uniform(-1.0, 1.0, (nz, ny, nx)).astype(np.float32)
    if kind == "ties":
        col = (np.round(col * 2.0) / 2.0).astype(np.float32)
    if kind == "nan":
        col[4, 6, 10] = col[0, 0, 0] = col[8, 11, 19] = col[3, 3, 0] = np.nan
    sh = abi.grid_shapes(nx, ny, nz)
    cv = [rng.uniform(-2.0, 2.0, sh[n]).astype(np.float32) for n in ("faceX", "faceY", "faceZ")]
    sc = abi.Scene(nx, ny, nz, 0.05, 1.0 / 24.0, 1000.0, [0.0, 0.0, 0.0], rng.uniform(-1.0, 1.0, (nz, ny, nx)), col, 1.0,
                   collisionvel=cv, name="box_" + kind)
    return sc, abi.default_params(tileSize=8, tilePadding=2, preconditioner=abi.PRE_DIAGONAL)


SCENES = {
    "blob": lambda: loads_cases.scene("blob"),
    "spheres32": lambda: loads_cases.scene("spheres32"),
    "box": lambda: box("random"),
    "box_ties": lambda: box("ties"),
    "box_nan": lambda: box("nan"),
}


def ids_field(sc, kind):
    if kind == "mod67":
        n = sc.nx * sc.ny * sc.nz
        return (np.arange(n, dtype=np.int64) % 67).astype(np.int32).reshape(sc.nz, sc.ny, sc.nx)
    return loads_cases.ids_field(sc, kind)


def table(kind, count, seed=7):
    """(count, 9): v, w, o per collider"""
    rng = np.random.RandomState(seed)
    t = np.zeros((count, 9), np.float64)
    if kind in ("translation", "both", "random"):
        t[:, 0:3] = rng.uniform(-1.5, 1.5, (count, 3))
    if kind in ("rotation", "both", "random"):
        t[:, 3:6] = rng.uniform(-6.0, 6.0, (count, 3))
        t[:, 6:9] = rng.uniform(-3.0, -1.0, (count, 3))            # a point off the grid
    if kind == "spheres":                                          # each sphere spins about its own centre and drifts
        t[:, 0:3] = rng.uniform(-1.0, 1.0, (count, 3))
        t[:, 3:6] = rng.uniform(-8.0, 8.0, (count, 3))
        t[:, 6:9] = np.array([c for c, _ in loads_cases.sphere_table()][:count])
    return t


# scene, id field, table kind, count, negateCollision, orig
CASES = {
    "blob_translation": ("blob", None, "translation", 1, 1, (0.0, 0.0, 0.0)),
    "blob_mod3_both": ("blob", "mod3", "both", 3, 1, (0.375, -1.25, 2.5)),
    "box_rotation": ("box", "mod3", "rotation", 2, 1, (0.0, 0.0, 0.0)),           # id 2 lies outside the count
    "box_count64": ("box", "mod67", "random", 64, 1, (-0.5, 0.25, 1.0)),          # ids 64 .. 66 lie outside
    "box_ties": ("box_ties", "mod3", "both", 3, 1, (0.0, 0.0, 0.0)),
    "box_nan": ("box_nan", "mod3", "both", 3, 1, (0.0, 0.0, 0.0)),
    "box_no_negate": ("box", "mod3", "both", 3, 0, (0.0, 0.0, 0.0)),
    "spheres_nearest": ("spheres32", "spheres", "spheres", 8, 1, (0.0, 0.0, 0.0)),
}
STEP_CASES = ("spheres_nearest", "blob_mod3_both")
_built = {}


def build(case):
    """(scene, params, ids, table, expected grids, expected counters); built once and shared: leave them unchanged"""
    if case not in _built:
        name, kind, tk, count, negate, orig = CASES[case]
        sc, p = SCENES[name]()
        sc.orig = orig
        p.negateCollision = negate
        ids, tab = ids_field(sc, kind), table(tk, count)
        grids, counters = ref.paint(sc.collision, ids, tab, orig, sc.dx, negate, sc.collisionvel)
        _built[case] = (sc, p, ids, tab, grids, counters)
    return _built[case]


def painted_scene(case):
    """the case's scene with the restatement's grids as collisionvel: what a fresh context is uploaded with"""
    sc, p, _, _, grids, _ = build(case)
    name = CASES[case][0]
    sc2, _ = SCENES[name]()
    sc2.orig = sc.orig
    sc2.collisionvel = [g.copy() for g in grids]
    return sc2, p


def digest(g):
    h = hashlib.sha256()
    for v in g:
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def upload_and_paint(s, case):
    sc, p, ids, tab, _, _ = build(case)
    s.upload(sc, p)
    if ids is not None:
        assert s.upload_collider_ids(ids) == abi.SUCCESS, s.last_error()
    assert s.paint_collider_velocities(tab) == abi.SUCCESS, s.last_error()


def painted(s):
    """(the three grids as (z, y, x) arrays, the counters) from the context's arrays"""
    sh = abi.grid_shapes(s.scene.nx, s.scene.ny, s.scene.nz)
    return [s.array(n).reshape(sh[f]) for n, f in zip(GRID_ARRAYS, ("faceX", "faceY", "faceZ"))], s.array("colliderMotionFaces")


def step_outcome(s):
    rc = s.step_device()
    s.download()
    return (int(rc), int(s.stats.result), int(s.stats.solveData[1]), [v.tobytes() for v in s.vel], [v.tobytes() for v in s.valid])


def outcome_digest(o):
    return digest([np.array(o[:3], np.int64)] + [np.frombuffer(b, np.uint8) for b in o[3] + o[4]])


if __name__ == "__main__" and len(sys.argv) >= 3 and sys.argv[1] == "paint":
    import polystokes_amd
    s = polystokes_amd.Solver(0)
    upload_and_paint(s, sys.argv[2])
    grids, counters = painted(s)
    print("DIGEST", digest(grids + [counters]), outcome_digest(step_outcome(s)))
    s.close()

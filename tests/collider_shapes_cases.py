"""Inputs shared by the collider-shape tests (test_collider_shapes_ref_cpu.py, test_gpu_collider_shapes.py), and the child process of the
switch tests:  python collider_shapes_cases.py place <case> ...  prints a digest of what a placement leaves in every named case.

The world is the 20 x 12 x 9 box of random SDF values of collider_motions_cases.py (partial blocks of 16 x 4 x 4 on all three axes, dx 0.05).
The volumes hold random values too: nothing here is meant to be a shape, every interpolation weight and every comparison matters.  Case
'lattice' alone takes dx = 1/16: with dx = 0.05 the world's cell centres (i + 0.5) * 0.05 are rounded, s_a misses the integers by a few
2^-53 and no f_a is exactly 0; with a power of two every step of the rule is exact and a won cell holds its sample."""
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
import collider_motions_cases as motions_cases  # noqa: E402
import collider_shapes_ref as ref  # noqa: E402

ARRAYS = ("colliderPlacement", "colliderPoseTable", "colliderPlacedCells", "collisionField", "colliderCellIds")
WORLD_CENTRE = np.array([0.5, 0.3, 0.225])     # of the 20 x 12 x 9 box at dx 0.05


def rotation(rng):
    """a random orthonormal R with determinant +1: the QR of a seeded matrix"""
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def volume(rng, n, h, lo=-1.0, hi=1.0):
    """(sdf (n2, n1, n0) of random values, h, a body-frame low corner that is not the volume's centre)"""
    sdf = rng.uniform(lo, hi, (n[2], n[1], n[0])).astype(np.float32)
    o = -0.5 * np.array(n, np.float64) * h + rng.uniform(-0.3, 0.3, 3)
    return sdf, float(h), o


def pose(shape, R, centre):
    """the 12 values that put the centre of the volume's box at `centre` (world)"""
    sdf, h, o = shape
    cb = np.asarray(o) + 0.5 * np.array(sdf.shape[::-1], np.float64) * h
    return np.concatenate([np.asarray(R, np.float64).ravel(), np.asarray(centre, np.float64) - R @ cb])


def three(orig):
    rng = np.random.RandomState(11)
    shapes = [volume(rng, (12, 10, 9), 0.04), volume(rng, (5, 4, 3), 0.06), volume(rng, (2, 2, 2), 0.11)]
    centres = [WORLD_CENTRE + (-0.1, 0.02, 0.0), WORLD_CENTRE + (0.12, -0.05, 0.05), WORLD_CENTRE + (0.0, 0.0, -0.02)]
    return shapes, np.array([pose(s, rotation(rng), c + np.asarray(orig)) for s, c in zip(shapes, centres)])


def lattice(orig):
    """same spacing, identity pose, origin on the world's lattice: sample (i, j, k) sits on cell (6 + i, 3 + j, 2 + k)"""
    rng = np.random.RandomState(5)
    sdf = rng.uniform(-1.0, 1.0, (5, 6, 8)).astype(np.float32)
    o = np.array([6, 3, 2], np.float64) * 0.0625
    return [(sdf, 0.0625, o)], np.concatenate([np.eye(3).ravel(), np.zeros(3)]).reshape(1, 12)


def count64(orig):
    """64 small volumes scattered over the box; every eighth lies wholly off the grid; 10 / 11 and 40 / 41 are identical pairs"""
    rng = np.random.RandomState(64)
    shapes, poses = [], []
    for k in range(64):
        n = tuple(int(q) for q in rng.randint(2, 5, 3))
        s = volume(rng, n, rng.uniform(0.03, 0.08))
        c = rng.uniform((0.0, 0.0, 0.0), (1.0, 0.6, 0.45))
        if k % 8 == 5:
            c = c + rng.choice([-1.0, 1.0], 3) * rng.uniform(2.0, 9.0, 3)
        shapes.append(s)
        poses.append(pose(s, rotation(rng), c))
    for k in (11, 41):
        shapes[k], poses[k] = shapes[k - 1], poses[k - 1].copy()
    return shapes, np.array(poses)


def larger(orig):
    rng = np.random.RandomState(4)
    s = volume(rng, (16, 12, 10), 0.1)
    return [s], pose(s, rotation(rng), WORLD_CENTRE).reshape(1, 12)


def spacings(orig):
    """h four times dx, and a quarter of it"""
    rng = np.random.RandomState(6)
    shapes = [volume(rng, (4, 3, 3), 0.2), volume(rng, (24, 20, 16), 0.0125)]
    centres = [WORLD_CENTRE + (0.1, 0.0, 0.0), WORLD_CENTRE + (-0.15, 0.05, 0.02)]
    return shapes, np.array([pose(s, rotation(rng), c) for s, c in zip(shapes, centres)])


# shapes and poses, id field, negateCollision, orig, what is done to the base collision, dx (None: the box's 0.05)
CASES = {
    "lattice": (lattice, None, 1, (0.0, 0.0, 0.0), None, 0.0625),
    "three_negate": (three, "mod3", 1, (0.0, 0.0, 0.0), None, None),
    "three_no_negate": (three, "mod3", 0, (0.0, 0.0, 0.0), None, None),
    "three_orig": (three, None, 1, (0.375, -1.25, 2.5), None, None),
    "count64": (count64, "mod3", 1, (0.0, 0.0, 0.0), None, None),
    "larger": (larger, None, 1, (0.0, 0.0, 0.0), None, None),
    "deep_base": (three, "mod3", 1, (0.0, 0.0, 0.0), "deep", None),
    "spacings": (spacings, None, 1, (0.0, 0.0, 0.0), None, None),
}
_built = {}


def build(case):
    """(scene, params, ids, shapes, poses, expected collision, expected ids, expected counters); built once and shared: leave them unchanged"""
    if case not in _built:
        make, kind, negate, orig, base, dx = CASES[case]
        sc, p = motions_cases.box("random")
        if dx is not None:
            sc.dx = dx
        if base == "deep":
            sc.collision = (sc.collision - np.float32(100.0)).astype(np.float32)     # D = -collision: deeper solid than any volume value
        sc.orig = orig
        p.negateCollision = negate
        ids = motions_cases.ids_field(sc, kind)
        shapes, poses = make(orig)
        col, idf, counters = ref.place(sc.collision, ids, shapes, poses, orig, sc.dx, negate)
        _built[case] = (sc, p, ids, shapes, poses, col, idf, counters)
    return _built[case]


def digest(g):
    h = hashlib.sha256()
    for v in g:
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def upload_and_place(s, case):
    sc, p, ids, shapes, poses = build(case)[:5]
    assert s.set_collider_shapes(shapes) == abi.SUCCESS, s.last_error()
    s.upload(sc, p)
    if ids is not None:
        assert s.upload_collider_ids(ids) == abi.SUCCESS, s.last_error()
    assert s.place_colliders(poses) == abi.SUCCESS, s.last_error()


def placed(s):
    """(collision (z, y, x), ids (z, y, x), counters) from the context's arrays"""
    sh = (s.scene.nz, s.scene.ny, s.scene.nx)
    return s.array("collisionField").reshape(sh), s.array("colliderCellIds").reshape(sh), s.array("colliderPlacedCells")


# ---- the stepping scene: spheres at 32^3 and two more spheres, as volumes, in the liquid ---------------------------------------------------
def sphere_volume(radius, n, h):
    """the SDF of a sphere (negative inside: the convention of a collision field with negateCollision = 1) about the centre of an n^3 volume"""
    q = (np.arange(n) + 0.5) * h - 0.5 * n * h
    z, y, x = np.meshgrid(q, q, q, indexing="ij")
    return (np.sqrt(x * x + y * y + z * z) - radius).astype(np.float32), float(h), np.full(3, -0.5 * n * h)


def step_scene():
    """(scene, params, shapes, poses, motions): the two volumes sit below the surface y = 0.5, turned by random rotations"""
    sc, p = scenes.spheres(32, tile=8)
    p.preconditioner = abi.PRE_DIAGONAL
    rng = np.random.RandomState(9)
    shapes = [sphere_volume(0.08, 12, 1.0 / 48.0), sphere_volume(0.06, 10, 1.0 / 56.0)]
    centres = [(0.27, 0.3, 0.31), (0.7, 0.36, 0.72)]
    poses = np.array([pose(s, rotation(rng), c) for s, c in zip(shapes, centres)])
    motions = np.zeros((2, 9))
    motions[:, 0:3] = rng.uniform(-1.0, 1.0, (2, 3))
    motions[:, 3:6] = rng.uniform(-4.0, 4.0, (2, 3))
    motions[:, 6:9] = centres
    return sc, p, shapes, poses, motions


def step_outcome(s):
    return motions_cases.step_outcome(s)


if __name__ == "__main__" and len(sys.argv) >= 3 and sys.argv[1] == "place":
    import polystokes_amd
    for case in sys.argv[2:]:
        s = polystokes_amd.Solver(0)
        upload_and_place(s, case)
        print("DIGEST", case, digest(placed(s)))
        s.close()

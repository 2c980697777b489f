"""Scenes, id fields and helpers shared by the collider-load tests (test_collider_loads_ref_cpu.py, test_gpu_collider_loads.py), and the
child process of the poisoned-buffer test:  python collider_loads_cases.py step <scene> <ids> <count>  prints the bytes of what a step leaves."""
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

import collider_loads_ref as ref  # noqa: E402

SCENES = {
    "blob": lambda: scenes.blob(24, 20, 28, tile=8),
    "spheres32": lambda: scenes.spheres(32, tile=8),
    "sliding32": lambda: scenes.sliding_block(32),
}
RESULT_ARRAYS = ("colliderForce", "colliderTorque", "colliderLoadTerms", "colliderLoadScale")


def scene(name):
    sc, p = SCENES[name]()
    p.preconditioner = abi.PRE_DIAGONAL
    return sc, p


def mirrored_scene(n=24):
    """A droplet falling onto a floor at rest, mirror-symmetric in x bit for bit: the SDF is the mean of itself and its mirror image, the
    floor does not depend on x, u_x is odd about the mid-plane (a spreading flow), u_y = -1.  In exact arithmetic F_x = 0."""
    dx, dt = 1.0 / n, 1.0 / 24.0
    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    x, y, z = (i + 0.5) * dx, (j + 0.5) * dx, (k + 0.5) * dx
    s = np.sqrt((x - 0.5) ** 2 + (y - 0.3) ** 2 + (z - 0.5) ** 2) - 0.25
    surface = (0.5 * (s + s[:, :, ::-1])).astype(np.float32)
    collision = (y - 2 * dx).astype(np.float32)
    u = np.broadcast_to(0.5 * (np.arange(n + 1) * dx - 0.5), (n, n, n + 1))
    ux = (0.5 * (u - u[:, :, ::-1])).astype(np.float32)
    sc = abi.Scene(n, n, n, dx, dt, 1000.0, [ux, -1.0, 0.0], surface, collision, 50.0, name="mirrored_droplet%d" % n)
    p = abi.default_params(tileSize=8, tilePadding=2, preconditioner=abi.PRE_DIAGONAL)
    return sc, p


def oracle_solution(o, x):
    """x (reference numbering) of an Oracle as the seven grids of ps_download_solution_fields: fp32, 0 without a DOF"""
    import helpers
    names = ("pressure", "txx", "tyy", "tzz", "tyz", "txz", "txy")
    return {name: np.nan_to_num(helpers.dof_field(o, kind, x, np.float64), nan=0.0).astype(np.float32) for name, kind in zip(names, helpers.DOF_KINDS)}


def cell_centres(sc):
    k, j, i = np.meshgrid(np.arange(sc.nz), np.arange(sc.ny), np.arange(sc.nx), indexing="ij")
    return (i + 0.5) * sc.dx, (j + 0.5) * sc.dx, (k + 0.5) * sc.dx


def sphere_table(nspheres=8, seed=12345):
    """centres and radii of scenes.spheres (the same draws in the same order)"""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(nspheres):
        c = rng.uniform(0.2, 0.8, 3)
        c[1] = rng.uniform(0.25, 0.55)
        rad = rng.uniform(0.06, 0.11)
        rng.uniform(-1.0, 1.0, 3)
        out.append((c, rad))
    return out


def ids_field(sc, kind):
    """None; 'mod3': linear cell index mod 3 (every wave holds three ids); 'spheres': the nearest sphere of scenes.spheres, 0..7, and the id 8
    — outside a count of 8 — on the low-x half of sphere 7's cells"""
    if kind is None or kind == "none":
        return None
    n = sc.nx * sc.ny * sc.nz
    if kind == "mod3":
        return (np.arange(n, dtype=np.int64) % 3).astype(np.int32).reshape(sc.nz, sc.ny, sc.nx)
    assert kind == "spheres", kind
    x, y, z = cell_centres(sc)
    tab = sphere_table()
    dist = np.stack([np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - rad for c, rad in tab])
    ids = np.argmin(dist, axis=0).astype(np.int32)
    ids[(ids == 7) & (x < tab[7][0][0])] = 8
    return ids


def pivots_for(sc, count, kind):
    """None (the upload's orig), or explicit points: the sphere centres, else points spread along the diagonal"""
    if kind is None:
        return None
    if kind == "spheres" and count <= 8:
        return np.array([c for c, _ in sphere_table()][:count], np.float64)
    return np.array([[0.1 + 0.07 * k, 0.5 - 0.03 * k, 0.25 + 0.05 * k] for k in range(count)], np.float64)


def got(s):
    """(F, T, counts, A, B) of the last step from its arrays"""
    n = int(s.array("colliderLoads")[0])
    scale = s.array("colliderLoadScale").reshape(n, 6)
    return (s.array("colliderForce").reshape(n, 3), s.array("colliderTorque").reshape(n, 3), s.array("colliderLoadTerms"),
            scale[:, :3].copy(), scale[:, 3:].copy())


def want(s, sc, count, ids=None, pivots=None, mutant=None):
    """the restatement fed the step's own arrays and solution_fields()"""
    return ref.loads(ref.inputs(s, sc, s.solution_fields()), count, ids, pivots, mutant)


def digest(g):
    h = hashlib.sha256()
    for v in g:
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def step(s, sc, p, count, ids=None, pivots=None):
    """upload, the setting, the ids, one step; returns the ps_result"""
    s.upload(sc, p)
    assert s.set_collider_loads(count, pivots) == abi.SUCCESS, s.last_error()
    if ids is not None:
        assert s.upload_collider_ids(ids) == abi.SUCCESS, s.last_error()
    return s.step_device()


if __name__ == "__main__" and len(sys.argv) >= 5 and sys.argv[1] == "step":
    import polystokes_amd
    name, kind, count = sys.argv[2], sys.argv[3], int(sys.argv[4])
    sc, p = scene(name)
    s = polystokes_amd.Solver(0)
    rc = step(s, sc, p, count, ids_field(sc, kind), pivots_for(sc, count, kind if kind == "spheres" else None))
    assert rc == abi.SUCCESS, rc
    print("DIGEST", digest(got(s)), digest([s.collider_loads()]))
    s.close()

"""The seeded cases of ps_advect_fields, shared by the CPU tests of the restatement (test_advection_ref_cpu.py) and the GPU tests
(test_gpu_advection.py).

Grids: scenes.blob(), 24 x 20 x 28 — not cubic, and 24 is no multiple of 16 — and 19 x 6 x 5: odd extents that are no multiples of the
16 x 4 x 4 block of the kernel and smaller than 16 along two axes; the upload takes it with tile = 8 (it only asks for positive extents).
Carriers: a seeded random one whose displacements reach 6 cells, so that departure points leave the grid on every side; a constant one of
exactly (2, -1, 3) cells per dt; one with an inf and a NaN sample; dt = 0; dt < 0.  The scene's own stepped velocity exists only on a GPU:
stepped_dt() chooses its dt there.
Cell fields: the scene's surface, a seeded random field whose magnitudes span twenty decades (a sum of a large and a small value loses the
small one even in fp64: that is what tells "l clamped" from "h clamped" at the upper border), and a linear ramp of small dyadic numbers."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from polystokes_amd import _abi as abi  # noqa: E402
from polystokes_amd import scenes  # noqa: E402
import advection_ref as ref  # noqa: E402

GRIDS = {"blob": (24, 20, 28), "odd": (19, 6, 5)}
CARRIERS = ("random", "shift", "nonfinite", "zero_dt", "negative_dt")
SHIFT = (2, -1, 3)               # cells per dt of the constant carrier, along x, y, z
_scenes, _built = {}, {}


def scene(grid):
    if grid not in _scenes:
        nx, ny, nz = GRIDS[grid]
        _scenes[grid] = scenes.blob(nx=nx, ny=ny, nz=nz, seed=3, tile=8)
    return _scenes[grid]


def face_shapes(dims):
    nx, ny, nz = dims
    return [(nz, ny, nx + 1), (nz, ny + 1, nx), (nz + 1, ny, nx)]


def carrier(grid, kind):
    """(the three face grids, dt)"""
    sc = scene(grid)[0]
    dims = GRIDS[grid]
    rng = np.random.RandomState({"blob": 11, "odd": 12}[grid] + 10 * CARRIERS.index(kind))
    dt = float(sc.dt)
    if kind == "shift":
        return [np.full(s, float(SHIFT[a]), np.float32) for a, s in enumerate(face_shapes(dims))], float(sc.dx)     # r = dx / dx = 1
    reach = {"random": 6.0, "nonfinite": 2.0, "zero_dt": 6.0, "negative_dt": 3.0}[kind]
    car = [(rng.uniform(-reach, reach, s) * sc.dx / dt).astype(np.float32) for s in face_shapes(dims)]
    if kind == "nonfinite":
        car[0][dims[2] // 2, dims[1] // 2, dims[0] // 2] = np.inf
        car[1][1, 2, 3] = np.nan
    if kind == "zero_dt":
        dt = 0.0
    if kind == "negative_dt":
        dt = -dt
    return car, dt


def cell_fields(grid):
    """[surface, random, ramp]"""
    sc = scene(grid)[0]
    nx, ny, nz = GRIDS[grid]
    rng = np.random.RandomState(5 + len(grid))
    wild = (rng.standard_normal((nz, ny, nx)) * 10.0 ** rng.uniform(-10.0, 10.0, (nz, ny, nx))).astype(np.float32)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ramp = (1.5 + 0.25 * i - 0.5 * j + 0.125 * k).astype(np.float32)
    return [np.ascontiguousarray(sc.surface, np.float32), wild, ramp]


def stepped_dt(sc, vel):
    """dt with max|u| dt / dx = 3.7 (nearly: the division rounds) for the velocity a step wrote"""
    top = max(float(np.abs(v[np.isfinite(v)]).max()) for v in vel)
    return 3.7 * float(sc.dx) / top


def reference(grid, kind, order, fields=3, velocity=True):
    """ref.advect of a case, computed once"""
    key = (grid, kind, order, fields, velocity)
    if key not in _built:
        car, dt = carrier(grid, kind)
        _built[key] = ref.advect(GRIDS[grid], float(scene(grid)[0].dx), dt, order, car, cell_fields(grid)[:fields], velocity)
    return _built[key]


def digest(cell_out, vel_out, counts, r):
    h = hashlib.sha256()
    for v in list(cell_out) + list(vel_out or []) + [np.asarray(counts, np.int32), np.asarray([r], np.float64)]:
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def run_host(s, grid, kind, order):
    """the case through ps_advect_fields on an uploaded context: (cell outputs, velocity outputs, counts, r)"""
    car, dt = carrier(grid, kind)
    rc, cout, vout = s.advect(dt, cell_fields(grid), order=order, carrier=car, velocity=True)
    assert rc == abi.SUCCESS, s.last_error()
    return cout, vout, s.array("advectionCounts"), float(s.array("advectionStep")[0])


if __name__ == "__main__" and len(sys.argv) >= 3 and sys.argv[1] == "advect":
    import polystokes_amd
    for name in sys.argv[2:]:
        grid, kind, order = name.split(":")
        s = polystokes_amd.Solver(0)
        s.upload(*scene(grid))
        print("DIGEST", name, digest(*run_host(s, grid, kind, int(order))))
        s.close()

"""The seeded cases of ps_advect_fields_scheme, shared by the CPU tests of the restatement (test_advection_scheme_ref_cpu.py) and the GPU tests
(test_gpu_advection_scheme.py).

Grids and cell fields are those of advection_cases.py: `blob` 24 x 20 x 28 and `odd` 19 x 6 x 5.  Carriers: its random, shift, nonfinite and
negative_dt ones and `gentle`, seed 77, uniform within +-GENTLE_REACH cells per dt: most departure and return points stay inside the grid, so
most samples take the corrected value.  On `odd` most samples fall back (the grid is a few cells thick): those cases are about block edges.

What the `blob` cases must show — else they would test the fallback, not the correction — is asserted on the restatement whenever
reference() builds one of them (every carrier but `shift`, whose correction is exactly zero), for each advected grid:
at most FALLBACK_CAP of the samples fall back; with a limiter, it changes at least one value; at least half the samples differ in bits from
the semi-Lagrangian result.  One case is outside these conditions and is said so here, not hidden: `random` at order 1.  Its Euler traces
reach 6 cells, and 0.52 / 0.51 / 0.53 / 0.49 of the samples of the cell / faceX / faceY / faceZ grids fall back (0.37 .. 0.38 at order 2,
where the conditions hold); that carrier belongs to advection_cases.py and stays as it is, so the case runs as a fallback case like `odd`."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import advection_cases as base  # noqa: E402
import advection_ref as ref  # noqa: E402
import advection_scheme_ref as sref  # noqa: E402
from polystokes_amd import _abi as abi  # noqa: E402

GRIDS = base.GRIDS
CARRIERS = ("random", "shift", "nonfinite", "negative_dt", "gentle")
LIMITERS = (sref.LIMIT_NONE, sref.LIMIT_CLAMP, sref.LIMIT_REVERT)
GENTLE_REACH = 1.5
FALLBACK_CAP = 0.45
scene, cell_fields, face_shapes = base.scene, base.cell_fields, base.face_shapes
_built = {}


def carrier(grid, kind):
    """(the three face grids, dt)"""
    if kind != "gentle":
        return base.carrier(grid, kind)
    sc = scene(grid)[0]
    rng = np.random.RandomState(77)
    dt = float(sc.dt)
    return [(rng.uniform(-GENTLE_REACH, GENTLE_REACH, s) * sc.dx / dt).astype(np.float32) for s in face_shapes(GRIDS[grid])], dt


def shares(grid, kind, order, limiter, got, sl):
    """per advected grid (samples, fallback share, values the limiter changed, share of samples whose bits differ from semi-Lagrangian)"""
    rows = []
    for g in range(4):
        new, old = (got[0], sl[0]) if g == 0 else ([got[1][g - 1]], [sl[1][g - 1]])
        differ = np.zeros(new[0].shape, bool)
        for a, b in zip(new, old):
            differ |= a.view(np.uint32) != b.view(np.uint32)
        rows.append((differ.size, int(got[4][4 + g]) / differ.size, int(got[4][g]), np.count_nonzero(differ) / differ.size))
    return rows


def reference(grid, kind, order, limiter, fields=3, velocity=True):
    """advection_scheme_ref.advect of a case, computed once"""
    key = (grid, kind, order, limiter, fields, velocity)
    if key not in _built:
        car, dt = carrier(grid, kind)
        got = sref.advect(GRIDS[grid], float(scene(grid)[0].dx), dt, order, car, cell_fields(grid)[:fields], velocity, limiter)
        if grid == "blob" and kind != "shift" and fields == 3 and velocity and (order == 2 or kind != "random"):
            sl = ref.advect(GRIDS[grid], float(scene(grid)[0].dx), dt, order, car, cell_fields(grid), True)
            for g, (n, fallback, limited, differ) in enumerate(shares(grid, kind, order, limiter, got, sl)):
                assert fallback <= FALLBACK_CAP, (key, g, fallback)
                assert limiter == sref.LIMIT_NONE or limited >= 1, (key, g, limited)
                assert differ >= 0.5, (key, g, differ)
        _built[key] = got
    return _built[key]


def digest(cell_out, vel_out, counts, r, correction):
    h = hashlib.sha256()
    for v in list(cell_out) + list(vel_out or []) + [np.asarray(counts, np.int32), np.asarray([r], np.float64), np.asarray(correction, np.int32)]:
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def what_the_call_left(s):
    return s.array("advectionCounts"), float(s.array("advectionStep")[0]), s.array("advectionCorrection")


def run_host(s, grid, kind, order, limiter):
    """the case through ps_advect_fields_scheme on an uploaded context: (cell outputs, velocity outputs, counts, r, correction)"""
    car, dt = carrier(grid, kind)
    rc, cout, vout = s.advect(dt, cell_fields(grid), order=order, carrier=car, velocity=True, scheme=abi.ADVECT_MACCORMACK, limiter=limiter)
    assert rc == abi.SUCCESS, s.last_error()
    return (cout, vout) + what_the_call_left(s)


if __name__ == "__main__" and len(sys.argv) >= 3 and sys.argv[1] == "advect":
    import polystokes_amd
    for name in sys.argv[2:]:
        grid, kind, order, limiter = name.split(":")
        s = polystokes_amd.Solver(0)
        s.upload(*scene(grid))
        print("DIGEST", name, digest(*run_host(s, grid, kind, int(order), int(limiter))))
        s.close()

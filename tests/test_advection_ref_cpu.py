"""The numpy restatement of the advection rule (advection_ref.py) on the shared cases (advection_cases.py), without a GPU: the cases tell the
rule from every near miss, dt = 0 copies, a whole-cell shift is exact, and no case is vacuous."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import advection_cases as cases  # noqa: E402
import advection_ref as ref  # noqa: E402

# the cases each mutant is meant for: (carrier, order)
MEANT = {
    "euler": [("random", 2), ("negative_dt", 2)],
    "cell_offset": [("random", 1), ("shift", 1)],
    "clamp_l": [("random", 1), ("random", 2)],
    "clamp_after_floor": [("random", 1)],
    "zyx": [("random", 1), ("negative_dt", 2)],
    "fp32": [("random", 2), ("negative_dt", 1)],
    "half_second": [("random", 2)],
    "nonfinite_index0": [("nonfinite", 1), ("nonfinite", 2)],
}


def _bytes(out):
    cells, vel, counts, r = out
    return b"".join(np.ascontiguousarray(v).tobytes() for v in list(cells) + list(vel) + [counts])


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_mutant_differs_from_the_rule(mutant):
    assert set(MEANT) == set(ref.MUTANTS)
    differs = []
    for grid in cases.GRIDS:
        for kind, order in MEANT[mutant]:
            car, dt = cases.carrier(grid, kind)
            got = ref.advect(cases.GRIDS[grid], float(cases.scene(grid)[0].dx), dt, order, car, cases.cell_fields(grid), True, mutant=mutant)
            differs.append(_bytes(got) != _bytes(cases.reference(grid, kind, order)))
    print(mutant, differs)
    assert any(differs)


@pytest.mark.parametrize("grid", sorted(cases.GRIDS))
@pytest.mark.parametrize("order", (1, 2))
def test_dt_zero_is_the_identity_on_the_bytes(grid, order):
    car, dt = cases.carrier(grid, "zero_dt")
    assert dt == 0.0
    cells, vel, counts, r = cases.reference(grid, "zero_dt", order)
    assert r == 0.0 and not counts.any()
    for got, want in zip(cells + vel, cases.cell_fields(grid) + car):
        assert got.tobytes() == want.tobytes()


def _shifted(out, src):
    """the interior of `out` and the samples of `src` a shift by SHIFT cells brings there"""
    sx, sy, sz = cases.SHIFT
    nz, ny, nx = src.shape
    m = 4                        # more than the largest shift: away from the clamped border
    if min(nz, ny, nx) <= 2 * m:
        return None
    return out[m:nz - m, m:ny - m, m:nx - m], src[m - sz:nz - m - sz, m - sy:ny - m - sy, m - sx:nx - m - sx]


@pytest.mark.parametrize("order", (1, 2))
def test_the_constant_carrier_shifts_exactly(order):
    grid = "blob"
    car, dt = cases.carrier(grid, "shift")
    cells, vel, counts, r = cases.reference(grid, "shift", order)
    assert r == 1.0 and counts[4] == 0 and (counts[:4] > 0).all()
    for got, src in zip(cells + vel, cases.cell_fields(grid) + car):
        a, b = _shifted(got, src)
        assert a.size > 100 and a.tobytes() == np.ascontiguousarray(b).tobytes()
    # the ramp: reproduced to 1 ulp of fp32 in the interior (here exactly, the shift being whole cells)
    ramp = cases.cell_fields(grid)[2]
    a, _ = _shifted(cells[2], ramp)
    nz, ny, nx = ramp.shape
    k, j, i = np.meshgrid(np.arange(4, nz - 4), np.arange(4, ny - 4), np.arange(4, nx - 4), indexing="ij")
    sx, sy, sz = cases.SHIFT
    want = 1.5 + 0.25 * (i - sx) - 0.5 * (j - sy) + 0.125 * (k - sz)
    assert (np.abs(a.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32))).all()


@pytest.mark.parametrize("grid", sorted(cases.GRIDS))
def test_the_cases_are_not_vacuous(grid):
    c1 = cases.reference(grid, "random", 1)
    c2 = cases.reference(grid, "random", 2)
    assert (c1[2][:4] > 0).all() and (c2[2][:4] > 0).all(), (c1[2], c2[2])
    assert _bytes(c1) != _bytes(c2)
    # the random carrier leaves the grid on every side
    car, dt = cases.carrier(grid, "random")
    p1, alone = ref.departure(cases.GRIDS[grid], 0, car, dt / float(cases.scene(grid)[0].dx), 1)
    for m, d in enumerate(cases.GRIDS[grid]):
        assert (p1[m] - 0.5 < 0).any() and (p1[m] - 0.5 > d - 1).any()
    assert np.abs(np.array(p1) - np.array(ref.departure(cases.GRIDS[grid], 0, [0 * c for c in car], 0.0, 1)[0])).max() > 4.0
    for order in (1, 2):
        n = cases.reference(grid, "nonfinite", order)[2]
        assert n[4] > 0, n
    # dt < 0 traces forward: the Euler displacement has the sign of the carrier there
    car, dt = cases.carrier(grid, "negative_dt")
    assert dt < 0 and cases.reference(grid, "negative_dt", 1)[3] < 0
    fwd = ref.departure(cases.GRIDS[grid], 0, car, dt / float(cases.scene(grid)[0].dx), 1)[0]
    rest = ref.departure(cases.GRIDS[grid], 0, car, 0.0, 1)[0]
    U = ref._carrier_at(cases.GRIDS[grid], car, rest, None, np.float64)
    for m in range(3):
        assert ((fwd[m] - rest[m]) * U[m] >= 0).all() and ((fwd[m] - rest[m]) * U[m] > 0).any()

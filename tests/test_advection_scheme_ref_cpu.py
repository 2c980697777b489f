"""The numpy restatement of the MacCormack rule (advection_scheme_ref.py) without a GPU: the shared cases tell the rule from each of its
near misses, the correction does what it is for on a translated Gaussian, the limiters keep a 0/1 box within [0, 1], and dt = 0 returns the
forward value."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import advection_ref as ref  # noqa: E402
import advection_scheme_cases as cases  # noqa: E402
import advection_scheme_ref as sref  # noqa: E402

N, STEPS, U = 32, 16, (0.37, -0.21, 0.43)      # the experiment of the header's author: 32^3, dx = dt = 1, a constant carrier, order 2
CENTRE = (10.0, 16.0, 14.0)


def _constant_carrier():
    return [np.full(s, U[a], np.float32) for a, s in enumerate(cases.face_shapes((N, N, N)))]


def _gaussian(shift):
    k, j, i = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    c = [CENTRE[m] + shift * np.float64(np.float32(U[m])) for m in range(3)]
    return np.exp(-((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2) / 18.0)


def _transport(field, limiter, steps=STEPS):
    """the field after `steps` steps; limiter None: semi-Lagrangian"""
    car = _constant_carrier()
    f = np.ascontiguousarray(field, np.float32)
    for _ in range(steps):
        if limiter is None:
            f = ref.advect((N, N, N), 1.0, 1.0, 2, car, [f])[0][0]
        else:
            f = sref.advect((N, N, N), 1.0, 1.0, 2, car, [f], False, limiter)[0][0]
    return f


def test_every_mutant_differs_from_the_rule_on_a_shared_case():
    report = {}
    for mutant in sref.MUTANTS:
        for grid, kind, order, limiter in (("blob", "gentle", 2, 1), ("blob", "random", 2, 2), ("odd", "gentle", 2, 1), ("blob", "negative_dt", 1, 1)):
            car, dt = cases.carrier(grid, kind)
            got = sref.advect(cases.GRIDS[grid], float(cases.scene(grid)[0].dx), dt, order, car, cases.cell_fields(grid), True, limiter, mutant=mutant)
            if cases.digest(*got) != cases.digest(*cases.reference(grid, kind, order, limiter)):
                report[mutant] = "%s:%s:%d:%d" % (grid, kind, order, limiter)
                break
    print("told apart on", report)
    assert sorted(report) == sorted(sref.MUTANTS), sorted(set(sref.MUTANTS) - set(report))


def test_the_correction_cuts_the_error_of_a_translated_gaussian():
    start, exact = _gaussian(0.0), _gaussian(float(STEPS))
    sl = _transport(start, None)
    l2_sl = float(np.sqrt(((sl - exact) ** 2).sum()))
    print("semi-Lagrangian l2 %.3f max %.3f peak %.3f" % (l2_sl, np.abs(sl - exact).max(), sl.max()))
    lo, hi = np.float32(start).min(), np.float32(start).max()
    for limiter in cases.LIMITERS:
        got = _transport(start, limiter)
        l2 = float(np.sqrt(((got - exact) ** 2).sum()))
        print("limiter %d l2 %.3f max %.3f peak %.3f ratio %.3f" % (limiter, l2, np.abs(got - exact).max(), got.max(), l2 / l2_sl))
        assert l2 <= 0.5 * l2_sl, (limiter, l2, l2_sl)
        if limiter == sref.LIMIT_CLAMP:
            assert got.max() <= hi and got.min() >= lo, (got.min(), lo, got.max(), hi)      # exact: a clamped value lies between samples


def test_the_limiters_keep_a_box_within_its_values():
    box = np.zeros((N, N, N), np.float32)
    box[9:19, 11:21, 8:18] = 1.0
    free = _transport(box, sref.LIMIT_NONE, 4)
    print("limiter none: min %.4f max %.4f" % (free.min(), free.max()))
    assert free.min() < 0.0 and free.max() > 1.0                                           # the correction overshoots at the box's faces
    for limiter in (sref.LIMIT_CLAMP, sref.LIMIT_REVERT):
        got = _transport(box, limiter, 4)
        print("limiter %d: min %.4f max %.4f" % (limiter, got.min(), got.max()))
        assert got.min() >= 0.0 and got.max() <= 1.0, limiter


def test_zero_dt_returns_the_forward_value_bit_for_bit():
    for grid in sorted(cases.GRIDS):
        car, _ = cases.carrier(grid, "random")
        dx = float(cases.scene(grid)[0].dx)
        for order in (1, 2):
            hat = ref.advect(cases.GRIDS[grid], dx, 0.0, order, car, cases.cell_fields(grid), True)
            for limiter in cases.LIMITERS:
                got = sref.advect(cases.GRIDS[grid], dx, 0.0, order, car, cases.cell_fields(grid), True, limiter)
                assert cases.digest(*got[:4], np.zeros(8, np.int32)) == cases.digest(*hat, np.zeros(8, np.int32)), (grid, order, limiter)
                assert not got[4].any()                                                   # nothing limited, nothing fell back

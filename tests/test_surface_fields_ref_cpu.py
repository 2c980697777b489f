"""The numpy restatement of the free-surface fields (tests/surface_fields_ref.py) on small synthetic label / weight grids: a constant
sigma field is the scalar formula, and a uniform ambient pressure is the negative of the liquid-side pressure gradient of the same
uniform pressure (the identity the GPU test of a uniform ambient pressure rests on)."""
import numpy as np
import pytest

from polystokes_amd import _abi as abi
import surface_fields_ref as ref


def _grid(seed, shape=(7, 6, 9), dyadic=False):
    """labels of every kind, liquid weights in [0, 1] with exact 0 and 1 among them, face weights with exact 0 among them, a curvature.
    dyadic: the weights are multiples of 1/64 (volume fractions of 4^3 samples), so that products with a power-of-two 1/dx are exact."""
    rng = np.random.RandomState(seed)
    nz, ny, nx = shape
    lab = rng.choice([abi.ACTIVEFLUID, abi.BOUNDARY, abi.REDUCED, abi.SOLID, abi.UNSOLVED, abi.GENERICFLUID], size=shape).astype(np.int32)
    q64 = lambda s: rng.randint(0, 65, size=s) / 64.0
    lw = (q64(shape) if dyadic else np.clip(rng.uniform(-0.3, 1.3, shape), 0, 1)).astype(np.float32)
    wf = []
    for s in ((nz, ny, nx + 1), (nz, ny + 1, nx), (nz + 1, ny, nx)):
        w = q64(s) if dyadic else np.clip(rng.uniform(-0.5, 1.2, s), 0, 1)
        wf.append(w.astype(np.float32))
    kappa = rng.uniform(-30, 30, shape).astype(np.float32)
    assert (lw == 0).any() and (lw == 1).any() and all((w == 0).any() for w in wf)
    return lab, lw, wf, kappa


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("v", [0.0, 0.07, 2.0])
def test_constant_sigma_field_is_the_scalar_formula(seed, v):
    lab, lw, wf, kappa = _grid(seed)
    dx, dt = 1.0 / 24, 1.0 / 30
    field = np.full(lab.shape, v, np.float32)
    q = ref.ghost_pressure(kappa, sigma_field=field)
    assert q.dtype == np.float64 and np.array_equal(q, float(np.float32(v)) * kappa.astype(np.float64))
    got = ref.ghost_sums(lab, lw, wf, q, dx)
    base = ref.ghost_sums(lab, lw, wf, kappa, dx)                       # sum g kappa
    # the largest single term g(f,c) sigma kappa_c dt: each face sum has two, each rounded a few times
    largest = dt * float(np.float32(v)) * max(np.abs(w).max() for w in wf) / dx * np.abs(kappa).max()
    for a in range(3):
        want = -dt * float(np.float32(v)) * base[a]
        assert np.abs(-dt * got[a] - want).max() <= 1e-12 * max(largest, 1e-300)
    # the scalar without a field gives the same q
    assert np.array_equal(ref.ghost_pressure(kappa, sigma=float(np.float32(v))), q)


def test_ghost_pressure_members():
    lab, lw, wf, kappa = _grid(2)
    rng = np.random.RandomState(5)
    s = rng.uniform(0, 2, lab.shape).astype(np.float32)
    P = rng.uniform(-500, 500, lab.shape).astype(np.float32)
    k64, s64, P64 = kappa.astype(np.float64), s.astype(np.float64), P.astype(np.float64)
    assert np.array_equal(ref.ghost_pressure(kappa, s, 0.0, P), s64 * k64 + P64)
    assert np.array_equal(ref.ghost_pressure(kappa, None, 1.5, P), 1.5 * k64 + P64)
    assert np.array_equal(ref.ghost_pressure(None, None, 0.0, P), P64)          # no curvature term at all


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_uniform_pressure_is_minus_the_liquid_side_gradient(seed):
    """ghost_c + liquid_c = 1 for every cell of the grid, so on a face with both cells in the grid the ghost term of a uniform P and the
    liquid-side gradient of the same P sum to wF (P - P) / dx = 0.  With weights in 1/64 and 1/dx a power of two every product is exact."""
    lab, lw, wf, _ = _grid(seed, dyadic=True)
    dx, P = 1.0 / 32, 1000.0
    val = np.full(lab.shape, P)
    ghost = ref.ghost_sums(lab, lw, wf, val, dx)
    liquid = ref.liquid_gradient(lab, lw, wf, val, dx)
    some = 0
    for a in range(3):
        ax = 2 - a
        inner = [slice(None)] * 3
        inner[ax] = slice(1, -1)                                         # faces whose two cells lie in the grid
        g, l = ghost[a][tuple(inner)], liquid[a][tuple(inner)]
        assert np.array_equal(g, -l)
        some += int((g != 0).sum())
        # a face on the grid border has one cell: there the ghost term is the whole one-sided coefficient times P, not minus the gradient
    assert some > 100

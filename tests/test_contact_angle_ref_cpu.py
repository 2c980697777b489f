"""The numpy restatement of the contact-angle rule (tests/contact_angle_ref.py), checked on its own: what it leaves alone, an axis-aligned
floor in closed form, the curvature it produces at the foot of a hemisphere and on a slanted wall, and a cut grid against the whole."""
import numpy as np
import pytest

import contact_angle_ref as ref


def _cos(deg):
    return 0.0 if deg == 90 else float(np.cos(deg * (np.pi / 180.0)))


def test_cells_outside_the_update_set_keep_their_bits():
    sc, _ = ref.hemisphere()
    out = ref.wetted(sc.surface, sc.collision, sc.dx, _cos(60))
    U = ref.update_set(sc.collision, sc.dx)
    assert U.sum() == 4 * 32 * 32                                        # the floor is 4 cells deep, all of it within 6 dx
    assert np.array_equal(out[~U].view(np.uint32), sc.surface[~U].view(np.uint32))
    assert (out[U] != sc.surface[U]).any()


def test_constant_depth_changes_nothing():
    surface, collision, dx = ref.crafted_constant()
    assert ref.update_set(collision, dx).all()
    out = ref.wetted(surface, collision, dx, _cos(30))
    assert np.array_equal(out.view(np.uint32), surface.view(np.uint32))


def test_column_without_an_upwind_cell_keeps_its_values():
    surface, collision, dx = ref.crafted_ramp()
    U = ref.update_set(collision, dx)
    assert U[:, :, :6].all() and not U[:, :, 6:].any()
    out = ref.wetted(surface, collision, dx, _cos(45))
    assert np.array_equal(out[:, :, 0].view(np.uint32), surface[:, :, 0].view(np.uint32))
    assert np.array_equal(out[:, :, 6:].view(np.uint32), surface[:, :, 6:].view(np.uint32))
    assert (out[:, :, 1:6] != surface[:, :, 1:6]).all()
    # column i takes column i - 1 minus dx cos, sweep by sweep: after 6 sweeps columns 1 .. 5 hang off column 0
    want = surface[:, :, 0].astype(np.float64)
    for i in range(1, 6):
        want = want - dx * _cos(45)
        assert np.abs(out[:, :, i] - want).max() <= 2e-6, i


@pytest.mark.parametrize("deg", [0, 60, 90, 120, 180])
def test_axis_aligned_floor(deg):
    """below an axis-aligned floor the only upwind cell is the one above: each solid layer equals the layer above it minus dx cos(theta)"""
    sc, _ = ref.hemisphere()
    out = ref.wetted(sc.surface, sc.collision, sc.dx, _cos(deg))
    for j in range(ref.HEMI_FLOOR - 1, -1, -1):
        want = (out[:, j + 1, :].astype(np.float64) - sc.dx * _cos(deg)).astype(np.float32)
        assert np.abs(out[:, j, :] - want).max() <= np.spacing(np.abs(want)).max(), j           # 1 ulp of fp32
    assert np.array_equal(out[:, ref.HEMI_FLOOR:, :], sc.surface[:, ref.HEMI_FLOOR:, :])


def _foot_mean(deg):
    sc, _ = ref.hemisphere()
    phi = sc.surface if deg is None else ref.wetted(sc.surface, sc.collision, sc.dx, _cos(deg))
    kap = ref.curvature(phi, sc.dx)
    foot = ref.hemisphere_foot(sc)
    assert foot.sum() > 100
    return kap, foot, float(kap[foot].astype(np.float64).mean())


def test_hemisphere_foot_curvature():
    two_over_r = 2.0 / ref.HEMI_R
    kap_off, foot, off = _foot_mean(None)
    assert abs(off / two_over_r - 1) <= 0.02, off
    kap90, _, m90 = _foot_mean(90)
    assert abs(m90 / two_over_r - 1) <= 0.02, m90                        # equilibrium kept
    _, _, m60 = _foot_mean(60)
    assert m60 < 0.5 * two_over_r, m60                                   # low pressure at the foot: it spreads
    _, _, m120 = _foot_mean(120)
    assert m120 > 1.5 * two_over_r, m120                                 # it retracts
    # far from the wall the curvature is that of the run without the rule, bit for bit: kappa_c reads within 7 cells of its cell
    far = np.zeros(kap_off.shape, bool)
    far[:, ref.HEMI_FLOOR + 7:, :] = True
    assert np.array_equal(kap90[far].view(np.uint32), kap_off[far].view(np.uint32))


@pytest.mark.parametrize("theta0", [50, 90, 130])
def test_slanted_wall(theta0):
    surface, collision, dx, foot = ref.slanted_wall(theta0)
    assert foot.sum() >= 32
    at = {}
    for d in (-30, 0, 30):
        kap = ref.curvature(ref.wetted(surface, collision, dx, _cos(theta0 + d)), dx).astype(np.float64)
        at[d] = kap[foot] * dx
    assert np.abs(at[0]).max() <= 1e-3, np.abs(at[0]).max()              # the angle the interface already has: flat stays flat
    assert at[-30].mean() < 0 < at[30].mean(), (at[-30].mean(), at[30].mean())


def test_cut_grid_matches_the_whole():
    """64^3 cut at z = 32 with 16 halo layers: kappa_c of each part equals the whole's on its owned cells plus one halo layer"""
    sc, _ = ref.cut_scene(64)
    c = _cos(60)
    whole = ref.curvature(ref.wetted(sc.surface, sc.collision, sc.dx, c), sc.dx)
    assert ref.update_set(sc.collision, sc.dx)[30:34, 5:, :].any()      # the solid sphere crosses the cut above the floor
    for lo, hi, own_lo, own_hi in ((0, 48, 0, 33), (16, 64, 31, 64)):
        part = ref.curvature(ref.wetted(sc.surface[lo:hi], sc.collision[lo:hi], sc.dx, c), sc.dx)
        assert np.array_equal(part[own_lo - lo:own_hi - lo].view(np.uint32), whole[own_lo:own_hi].view(np.uint32)), (lo, hi)

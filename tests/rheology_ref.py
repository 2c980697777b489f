"""numpy restatement of the non-Newtonian viscosity of ps_set_rheology (include/polystokes.h, ps_rheology.hip).

Arrays are numpy grids in (z, y, x) order, x fastest (_abi.grid_shapes): axis a of the solver (0 = x) is numpy axis 2 - a.  `used[a]` is the
boolean face grid of the used samples of axis a: the `valid` output of the same step (label neither UNSOLVED nor UNASSIGNED)."""
import numpy as np


def _sl(ax, lo, hi):
    s = [slice(None)] * 3
    s[ax] = slice(lo, hi)
    return tuple(s)


def _central(u, used, b, dx):
    """du/dx_b at every face of one face grid and where it exists (both neighbours along b inside the grid and used)"""
    ax = 2 - b
    n = u.shape[ax]
    val = np.zeros(u.shape, np.float64)
    has = np.zeros(u.shape, bool)
    if n >= 3:
        lo, hi = _sl(ax, 0, n - 2), _sl(ax, 2, n)
        mid = _sl(ax, 1, n - 1)
        h = used[lo] & used[hi]
        val[mid] = np.where(h, (u[hi] - u[lo]) / (2.0 * dx), 0.0)
        has[mid] = h
    return val, has


def masks_and_gradients(vel, used, dx):
    """D_aa, G_ab (key (a, b)) on the cell grid, with the masks: pair[a] (both a-faces of the cell used) and has[(a, b)] (G_ab exists)"""
    D, pair, G, has = {}, {}, {}, {}
    for a in range(3):
        u = np.asarray(vel[a], np.float32).astype(np.float64)
        m = np.asarray(used[a], bool)
        ax = 2 - a
        n = u.shape[ax] - 1
        f0, f1 = _sl(ax, 0, n), _sl(ax, 1, n + 1)
        pair[a] = m[f0] & m[f1]
        D[a] = np.where(pair[a], (u[f1] - u[f0]) / dx, 0.0)
        for b in range(3):
            if b == a:
                continue
            cd, h = _central(u, m, b, dx)
            g0, g1, h0, h1 = cd[f0], cd[f1], h[f0], h[f1]
            G[(a, b)] = np.where(h0 & h1, 0.5 * (g0 + g1), np.where(h0, g0, np.where(h1, g1, 0.0)))
            has[(a, b)] = h0 | h1
    return D, G, pair, has


def strain_rate(vel, used, dx):
    """gammaDot_c = sqrt(2 sum_a D_aa^2 + 4 sum_{a<b} D_ab^2), D_ab = (G_ab + G_ba) / 2, in fp64"""
    D, G, _, _ = masks_and_gradients(vel, used, dx)
    Dxy = 0.5 * (G[(0, 1)] + G[(1, 0)])
    Dxz = 0.5 * (G[(0, 2)] + G[(2, 0)])
    Dyz = 0.5 * (G[(1, 2)] + G[(2, 1)])
    return np.sqrt(2.0 * (D[0] * D[0] + D[1] * D[1] + D[2] * D[2]) + 4.0 * (Dxy * Dxy + Dxz * Dxz + Dyz * Dyz))


def viscosity(rate, K, n, tau_y, min_rate, min_visc, max_visc):
    """mu = min(max(K s^(n-1) + tau_y / s, min_visc), max_visc), s = max(rate, min_rate); n == 1 skips the power"""
    s = np.maximum(rate, min_rate)
    K = np.asarray(K, np.float32).astype(np.float64)
    m = (K if n == 1.0 else K * np.power(s, n - 1.0)) + tau_y / s
    return np.minimum(np.maximum(m, min_visc), max_visc)


def fields(scene_vel, valid, dx, K, n, tau_y, min_rate, min_visc, max_visc):
    """(gammaDot, mu) as the library stores them (fp32) from a velocity and the step's valid flags"""
    rate = strain_rate(scene_vel, [np.asarray(v) > 0 for v in valid], float(np.float32(dx)))
    mu = viscosity(rate, K, n, tau_y, min_rate, min_visc, max_visc)
    return rate.astype(np.float32), mu.astype(np.float32)


def ulps(a, b):
    """fp32 ulp distance, elementwise (both finite)"""
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)

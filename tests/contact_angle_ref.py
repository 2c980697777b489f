"""numpy restatement of the contact-angle rule (include/polystokes.h, ps_set_contact_angle): the liquid SDF rewritten inside the solid so
that its slope along the wall normal is cos(theta), in the library's order of operations (fp64 from the fp32 inputs, unfused), plus the
scenes and measures the CPU and GPU tests share.  The curvature applied to the result is the restatement of
tests/test_gpu_surface_tension.py.  Arrays are (nz, ny, nx), x fastest."""
import numpy as np

from polystokes_amd import _abi as abi
from polystokes_amd import scenes

SWEEPS = abi.CONTACT_ANGLE_SWEEPS


def curvature(phi, dx):
    """kappa_c of ps_set_surface_tension for the SDF phi (the existing numpy restatement)"""
    from test_gpu_surface_tension import _curvature
    return _curvature(np.asarray(phi, np.float32), dx)


def depth(collision, negate=1):
    """D_c in fp32: -collision with negateCollision = 1, +collision with 0 (positive inside the solid)"""
    c = np.asarray(collision, np.float32)
    return -c if negate else c


def update_set(collision, dx, negate=1):
    """U = { c : D_c > 0 and (double)D_c <= 6.0 * dx }"""
    D = depth(collision, negate)
    return (D > 0) & (D.astype(np.float64) <= 6.0 * float(dx))


def _neighbours(f, ax):
    """(value at c - e, it exists, value at c + e, it exists) along numpy axis ax; a missing neighbour reads 0 and is never used"""
    n = f.shape[ax]
    lo, hi = np.zeros_like(f), np.zeros_like(f)
    has_lo, has_hi = np.zeros(f.shape, bool), np.zeros(f.shape, bool)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    src[ax], dst[ax] = slice(0, n - 1), slice(1, n)
    lo[tuple(dst)] = f[tuple(src)]
    has_lo[tuple(dst)] = True
    hi[tuple(src)] = f[tuple(dst)]
    has_hi[tuple(src)] = True
    return lo, has_lo, hi, has_hi


def wetted(surface, collision, dx, cos, negate=1, sweeps=SWEEPS):
    """phi' = phi^sweeps as fp32.  cos: the scalar's cosine (a float) or the fp32 cell field."""
    dx = float(dx)
    phi = np.array(surface, np.float32, copy=True)
    D = depth(collision, negate).astype(np.float64)
    U = update_set(collision, dx, negate)
    pad = np.pad(D, 1, mode="edge")                                    # indices clamped to the grid
    G = [(pad[1:-1, 1:-1, 2:] - pad[1:-1, 1:-1, :-2]) * 0.5,
         (pad[1:-1, 2:, 1:-1] - pad[1:-1, :-2, 1:-1]) * 0.5,
         (pad[2:, 1:-1, 1:-1] - pad[:-2, 1:-1, 1:-1]) * 0.5]
    g = np.sqrt(G[0] * G[0] + G[1] * G[1] + G[2] * G[2])
    cosd = float(cos) if np.ndim(cos) == 0 else np.asarray(cos, np.float32).astype(np.float64).reshape(phi.shape)
    drop = (dx * cosd) * g
    for _ in range(sweeps):
        f = phi.astype(np.float64)
        N, W = np.zeros_like(f), np.zeros_like(f)
        for a in range(3):                                              # x, y, z: numpy axes 2, 1, 0
            lo, has_lo, hi, has_hi = _neighbours(f, 2 - a)
            w = np.abs(G[a])
            use_lo, use_hi = (G[a] > 0) & has_lo, (G[a] < 0) & has_hi   # the upwind cell: toward the wall, inside the grid
            up = np.where(use_lo, lo, hi)
            used = use_lo | use_hi
            N = np.where(used, N + w * up, N)
            W = np.where(used, W + w, W)
        moved = U & (W != 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            new = ((N - drop) / np.where(moved, W, 1.0)).astype(np.float32)
        phi = np.where(moved, new, phi)
    return phi


# ---- scenes ---------------------------------------------------------------------------------------------------------------
HEMI_N, HEMI_R, HEMI_FLOOR = 32, 0.3, 4


def hemisphere(sigma=None, angle=None):
    """the hemisphere on a floor of the issue: 32^3, radius 0.3, the floor plane 4 cells up (2 / R = 6.667)"""
    return scenes.sessile_drop(HEMI_N, HEMI_R, HEMI_FLOOR, sigma=sigma, contact_angle=angle)


def hemisphere_foot(sc):
    """the liquid cells of the two layers above the floor that lie within 1.5 dx of the interface"""
    m = np.zeros(sc.surface.shape, bool)
    m[:, HEMI_FLOOR:HEMI_FLOOR + 2, :] = True
    return m & (sc.surface < 0) & (np.abs(sc.surface) < 1.5 * sc.dx)


def slanted_wall(theta0, n=32):
    """(surface, collision, dx, foot): a plane wall through the centre line x = y = 0.5 whose normal into the fluid is
    (sin theta0, cos theta0, 0), and a flat interface y = 0.5 with the liquid below it, which meets the wall at theta0 inside the liquid.
    foot: liquid cells within 2 dx of the wall and 1.5 dx of the interface."""
    dx = 1.0 / n
    t = np.deg2rad(theta0)
    c = (np.arange(n) + 0.5) * dx
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    surface = (y - 0.5).astype(np.float32)
    collision = (np.sin(t) * (x - 0.5) + np.cos(t) * (y - 0.5)).astype(np.float32)     # negative inside the solid
    foot = (collision > 0) & (collision < 2 * dx) & (surface < 0) & (np.abs(surface) < 1.5 * dx)
    return surface, collision, dx, foot


def crafted_constant(n=12):
    """D constant (inside the band): every gradient is 0, so nothing changes"""
    dx = 1.0 / n
    rng = np.random.RandomState(5)
    surface = rng.uniform(-1, 1, (n, n, n)).astype(np.float32)
    collision = np.full((n, n, n), -2.5 * dx, np.float32)
    return surface, collision, dx


def crafted_ramp(n=12):
    """D = x + 0.5 dx with x = i dx (solid everywhere): the upwind cell is c - e_x, which column 0 lacks.  Columns 0 .. 5 lie in the band."""
    dx = 1.0 / n
    rng = np.random.RandomState(6)
    surface = rng.uniform(-1, 1, (n, n, n)).astype(np.float32)
    D = (np.arange(n) * dx + 0.5 * dx).astype(np.float32)
    collision = np.broadcast_to(-D, (n, n, n)).copy()
    return surface, collision, dx


def cut_scene(n=64):
    """a liquid hemisphere on a floor (the wall hemisphere) plus a solid sphere across the plane z = n / 2, for the decomposition checks"""
    sc, p = scenes.sessile_drop(n, 0.3, 4, tile=8)
    c = (np.arange(n) + 0.5) * sc.dx
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    ball = np.sqrt((x - 0.62) ** 2 + (y - 0.2) ** 2 + (z - 0.5) ** 2) - 0.09
    sc.collision[:] = np.minimum(sc.collision, ball.astype(np.float32))
    return sc, p

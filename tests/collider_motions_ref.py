"""The rule of ps_paint_collider_velocities (include/polystokes.h) restated in numpy.  Arrays are (z, y, x) as everywhere in the tests: axis a
of the rule is numpy axis 2 - a.  All arithmetic is fp64 from the fp32 / fp64 inputs, elementwise (numpy fuses nothing), in the order the
header writes it, so the device's grids are expected byte for byte.

MUTANTS are near misses of the rule, switched on by name; test_collider_motions_ref_cpu.py shows that the cases tell each from the rule."""
import numpy as np

# tie_upper: D_U >= D_L picks the upper cell; swap_a1_a2: the cross product with its two transverse axes exchanged; line_transverse: the
# transverse coordinates on grid lines instead of cell centres; id_less_solid: the id of the cell that lost the comparison.
# centre_along_a is the header's "cell centre instead of grid line along a": the painted component a of w x arm does not contain arm[a], so
# it can change nothing; it is kept to pin exactly that.
MUTANTS = ("tie_upper", "swap_a1_a2", "line_transverse", "id_less_solid")
NEUTRAL_MUTANTS = ("centre_along_a",)


def face_shape(shape_zyx, a):
    s = list(shape_zyx)
    s[2 - a] += 1
    return tuple(s)


def chosen_cells(collision, a, negate=1, mutant=None):
    """per face of axis a: the (k, j, i) index arrays of the chosen cell, and those of the other cell (the chosen one again where only one exists)"""
    D = -collision if negate else collision
    ax = 2 - a
    n = collision.shape[ax]
    idx = list(np.indices(face_shape(collision.shape, a)))
    ia = idx[ax]
    lo, up = np.clip(ia - 1, 0, n - 1), np.clip(ia, 0, n - 1)

    def cell(along):
        c = list(idx)
        c[ax] = along
        return tuple(c)
    DL, DU = D[cell(lo)], D[cell(up)]
    both = (ia >= 1) & (ia <= n - 1)
    with np.errstate(invalid="ignore"):
        upper_wins = DU >= DL if mutant == "tie_upper" else DU > DL          # a NaN compares false: the lower cell
    use_up = np.where(both, upper_wins, ia == 0)
    return cell(np.where(use_up, up, lo)), cell(np.where(use_up, lo, up))


def paint(collision, ids, table, orig, dx, negate=1, cvel=None, mutant=None):
    """collision: fp32 (nz, ny, nx); ids: int32 cell field or None; table: (count, 9) fp64; cvel: the three uploaded grids (None: zeros).
    Returns ([gx, gy, gz] fp32: painted, or the uploaded value where left alone; int32 counters of count + 2)."""
    collision = np.asarray(collision, np.float32)
    table = np.asarray(table, np.float64).reshape(-1, 9)
    count = table.shape[0]
    finite = np.isfinite(table).all(axis=1)
    counters = np.zeros(count + 2, np.int64)
    out = []
    for a in range(3):
        a1, a2 = (a + 1) % 3, (a + 2) % 3
        if mutant == "swap_a1_a2":
            a1, a2 = a2, a1
        shape = face_shape(collision.shape, a)
        chosen, other = chosen_cells(collision, a, negate, mutant)
        src = other if mutant == "id_less_solid" else chosen
        k = np.zeros(shape, np.int64) if ids is None else np.asarray(ids)[src].astype(np.int64)
        known = (k >= 0) & (k < count)
        kk = np.where(known, k, 0)
        painted = known & finite[kk]
        idx = np.indices(shape)
        r = []
        for m in range(3):
            i_m = idx[2 - m].astype(np.float64)
            on_line = (m == a) if mutant != "line_transverse" else True
            if mutant == "centre_along_a":
                on_line = False
            r.append(float(orig[m]) + (i_m if on_line else i_m + 0.5) * float(dx))
        v, w, o = table[kk, 0:3], table[kk, 3:6], table[kk, 6:9]
        with np.errstate(invalid="ignore", over="ignore"):
            arm1, arm2 = r[a1] - o[..., a1], r[a2] - o[..., a2]
            value = (v[..., a] + (w[..., a1] * arm2 - w[..., a2] * arm1)).astype(np.float32)
        before = np.zeros(shape, np.float32) if cvel is None else np.asarray(cvel[a], np.float32)
        out.append(np.where(painted, value, before).astype(np.float32))
        counters[:count] += np.bincount(k[painted], minlength=count)
        counters[count] += int((~known).sum())
        counters[count + 1] += int((known & ~painted).sum())
    return out, counters.astype(np.int32)


def divergence(grids, dx):
    """the discrete divergence per cell, fp64 from the fp32 grids"""
    gx, gy, gz = (np.asarray(g, np.float64) for g in grids)
    return ((gx[:, :, 1:] - gx[:, :, :-1]) + (gy[:, 1:, :] - gy[:, :-1, :]) + (gz[1:, :, :] - gz[:-1, :, :])) / dx

"""ps_set_velocity_extrapolation restated in numpy (include/polystokes.h): on one face grid, L = 0 on valid faces and -1 elsewhere; sweep k
gives every face with L == -1 that has a 6-neighbour with 0 <= L < k the fp32 rounding of the fp64 mean of those neighbours (summed in the
order -x, +x, -y, +y, -z, +z from 0) and L = k.  Jacobi sweeps: a sweep reads the state the sweep before it left.

Arrays are (z, y, x) like every field of the harness.  The keyword arguments after `layers` exist for tests/test_extrapolation_ref_cpu.py,
which checks that the inputs of the GPU comparison tell the rule from its near misses; the rule itself is the call without them."""
import numpy as np

# (axis of the (z, y, x) array, offset of the neighbour): -x, +x, -y, +y, -z, +z
DIRECTIONS = ((2, -1), (2, +1), (1, -1), (1, +1), (0, -1), (0, +1))


def _pair(shape, axis, off):
    """(destination slice, source slice): destination face f and its neighbour f + off along `axis`, where both lie inside the grid"""
    dst, src = [slice(None)] * 3, [slice(None)] * 3
    if off < 0:
        dst[axis], src[axis] = slice(1, None), slice(0, shape[axis] - 1)
    else:
        dst[axis], src[axis] = slice(0, shape[axis] - 1), slice(1, None)
    return tuple(dst), tuple(src)


def extrapolate(vel_zyx, valid_zyx, layers, directions=DIRECTIONS, acc=np.float64):
    """-> (vel fp32, L int8, counts int32 of length `layers`: the faces each sweep assigned)."""
    vel = np.array(vel_zyx, dtype=np.float32, copy=True)
    L = np.where(np.asarray(valid_zyx) == 1, 0, -1).astype(np.int8)
    assert vel.shape == L.shape and vel.ndim == 3
    counts = np.zeros(int(layers), np.int32)
    for k in range(1, int(layers) + 1):
        known = L >= 0                                  # every layer assigned so far is below k
        total = np.zeros(vel.shape, acc)
        count = np.zeros(vel.shape, np.int32)
        for axis, off in directions:
            dst, src = _pair(vel.shape, axis, off)
            m = known[src]
            t = total[dst]
            t[m] = t[m] + vel[src][m].astype(acc)       # one rounded addition per neighbour, in this order
            total[dst] = t
            count[dst] += m
        new = (L == -1) & (count > 0)
        vel[new] = (total[new] / count[new].astype(acc)).astype(np.float32)
        L[new] = k
        counts[k - 1] = int(new.sum())
    return vel, L, counts


def extrapolate_sequential(vel_zyx, valid_zyx, layers, same_sweep=False):
    """The rule one face at a time in flat (x fastest) order, without numpy's shifted views.  same_sweep = False is the rule; True accepts a
    neighbour assigned earlier in the same sweep (a Gauss-Seidel sweep: what an in-place kernel without the L < k test would compute)."""
    vel = np.array(vel_zyx, dtype=np.float32, copy=True)
    nz, ny, nx = vel.shape
    v = vel.reshape(-1)
    L = np.where(np.asarray(valid_zyx).reshape(-1) == 1, 0, -1).astype(np.int8)
    counts = np.zeros(int(layers), np.int32)
    sy, sz = nx, nx * ny
    for k in range(1, int(layers) + 1):
        before = L.copy()
        src_L = L if same_sweep else before
        top = k if same_sweep else k - 1
        for c in np.flatnonzero(before == -1):
            i, j, kk = c % nx, (c // nx) % ny, c // sz
            total, n = np.float64(0.0), 0
            for inside, f in ((i > 0, c - 1), (i + 1 < nx, c + 1), (j > 0, c - sy), (j + 1 < ny, c + sy), (kk > 0, c - sz), (kk + 1 < nz, c + sz)):
                if inside and 0 <= src_L[f] <= top:
                    total = total + np.float64(v[f])
                    n += 1
            if n:
                v[c] = np.float32(total / np.float64(n))
                L[c] = k
                counts[k - 1] += 1
    return vel, L.reshape(vel.shape), counts

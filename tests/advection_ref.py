"""The rule of ps_advect_fields (include/polystokes.h "Advection") restated in numpy: fp64 from the fp32 inputs, no fused step, every
operation in the order the header writes it.  Arrays are (z, y, x) like every host array of the harness; a point p is the list (p_x, p_y, p_z).

MUTANTS names the near misses the shared cases must tell from the rule (test_advection_ref_cpu.py): advect(..., mutant=name) computes that one."""
import numpy as np

MUTANTS = ("euler",              # Euler where midpoint is asked
           "cell_offset",        # the cell offset 0.5 on a face grid's own axis
           "clamp_l",            # l clamped to d - 2 (h = l + 1) instead of h clamped
           "clamp_after_floor",  # floor(s) first, the index clamped afterwards: the fraction survives outside the grid
           "zyx",                # interpolation along z, then y, then x
           "fp32",               # the arithmetic in fp32
           "half_second",        # r * 0.5 applied to the second stage too
           "nonfinite_index0")   # a non-finite point sampled as index 0 instead of left alone
QUIET_NAN = np.uint32(0x7fc00000)
SLOTS = 5                        # clamped samples of the cell, faceX, faceY, faceZ grids; samples left alone


def extents(dims, g):
    """(d_x, d_y, d_z) of grid kind g: 0 cell, 1 faceX, 2 faceY, 3 faceZ"""
    d = list(dims)
    if g > 0:
        d[g - 1] += 1
    return d


def offsets(g, mutant=None):
    o = [0.5, 0.5, 0.5]
    if g > 0 and mutant != "cell_offset":
        o[g - 1] = 0.0
    return o


def _taps(dims, g, p, mutant, T):
    """per axis (l, h, f) of the sampler of grid g at the finite points p, and whether a point left the grid"""
    d, o = extents(dims, g), offsets(g, mutant)
    taps, clamped = [], np.zeros(p[0].shape, bool)
    for m in range(3):
        s = p[m] - T(o[m])
        top = T(d[m] - 1)
        if mutant == "clamp_after_floor":
            fl = np.floor(s)
            l = np.minimum(np.maximum(fl, T(0)), top).astype(np.int64)
            h = np.minimum(l + 1, d[m] - 1)
            f = s - fl
        else:
            c = np.minimum(np.maximum(s, T(0)), top)
            l = np.floor(c).astype(np.int64)
            if mutant == "clamp_l":
                l = np.minimum(l, d[m] - 2)
                h = l + 1
            else:
                h = np.minimum(l + 1, d[m] - 1)
            f = c - l.astype(T)
        taps.append((l, h, f))
        clamped |= (s < 0) | (s > top)
    return taps, clamped


def _gather(F, taps, mutant, T):
    (lx, hx, fx), (ly, hy, fy), (lz, hz, fz) = taps
    v = lambda z, y, x: F[z, y, x].astype(T)
    lerp = lambda lo, hi, f: lo + (hi - lo) * f
    if mutant == "zyx":
        z00, z10 = lerp(v(lz, ly, lx), v(hz, ly, lx), fz), lerp(v(lz, ly, hx), v(hz, ly, hx), fz)
        z01, z11 = lerp(v(lz, hy, lx), v(hz, hy, lx), fz), lerp(v(lz, hy, hx), v(hz, hy, hx), fz)
        return lerp(lerp(z00, z01, fy), lerp(z10, z11, fy), fx)
    x00, x10 = lerp(v(lz, ly, lx), v(lz, ly, hx), fx), lerp(v(lz, hy, lx), v(lz, hy, hx), fx)
    x01, x11 = lerp(v(hz, ly, lx), v(hz, ly, hx), fx), lerp(v(hz, hy, lx), v(hz, hy, hx), fx)
    return lerp(lerp(x00, x10, fy), lerp(x01, x11, fy), fz)


def _carrier_at(dims, carrier, p, mutant, T):
    return [_gather(carrier[a], _taps(dims, 1 + a, p, mutant, T)[0], mutant, T) for a in range(3)]


def _finite_or_alone(p, alone, mutant, T):
    """the points with every coordinate finite kept, the others marked left alone and given a stand-in that is never used (the mutant
    samples them as index 0)"""
    bad = ~(np.isfinite(p[0]) & np.isfinite(p[1]) & np.isfinite(p[2]))
    if mutant == "nonfinite_index0":
        return [np.where(np.isfinite(q), q, T(0)) for q in p], alone
    alone = alone | bad
    return [np.where(alone, T(0), q) for q in p], alone


def departure(dims, g, carrier, r, order, mutant=None):
    """(p1, alone) for every sample of grid g"""
    T = np.float32 if mutant == "fp32" else np.float64
    d, o = extents(dims, g), offsets(g, mutant)
    k, j, i = np.meshgrid(np.arange(d[2]), np.arange(d[1]), np.arange(d[0]), indexing="ij")
    p0 = [i.astype(T) + T(o[0]), j.astype(T) + T(o[1]), k.astype(T) + T(o[2])]
    r = T(r)
    alone = np.zeros(p0[0].shape, bool)
    U = _carrier_at(dims, carrier, p0, mutant, T)
    step = r
    if order == 2 and mutant != "euler":
        half = T(0.5) * r
        pm, alone = _finite_or_alone([p0[m] - half * U[m] for m in range(3)], alone, mutant, T)
        U = _carrier_at(dims, carrier, pm, mutant, T)
        if mutant == "half_second":
            step = half
    p1, alone = _finite_or_alone([p0[m] - step * U[m] for m in range(3)], alone, mutant, T)
    return p1, alone


def _stored(v, source, alone):
    out = v.astype(np.float32)
    bits = np.where(np.isnan(v), QUIET_NAN, out.view(np.uint32))
    return np.where(alone, source.view(np.uint32), bits).astype(np.uint32).view(np.float32)


def advect(dims, dx, dt, order, carrier, cell_in=(), velocity=False, mutant=None):
    """(cell outputs, velocity outputs or None, counts int32[5], r).  dims = (nx, ny, nz); carrier: the three face grids; dx, dt: what the
    upload and the call hold, as doubles."""
    T = np.float32 if mutant == "fp32" else np.float64
    carrier = [np.ascontiguousarray(c, np.float32) for c in carrier]
    r = np.float64(dt) / np.float64(dx)
    counts = np.zeros(SLOTS, np.int64)
    cell_out, vel_out = [], None
    with np.errstate(all="ignore"):
        if len(cell_in):
            p1, alone = departure(dims, 0, carrier, r, order, mutant)
            taps, clamped = _taps(dims, 0, p1, mutant, T)
            counts[0] += np.count_nonzero(clamped & ~alone)
            counts[4] += np.count_nonzero(alone)
            for F in cell_in:
                F = np.ascontiguousarray(F, np.float32)
                cell_out.append(_stored(_gather(F, taps, mutant, T), F, alone))
        if velocity:
            vel_out = []
            for a in range(3):
                p1, alone = departure(dims, 1 + a, carrier, r, order, mutant)
                taps, clamped = _taps(dims, 1 + a, p1, mutant, T)
                counts[1 + a] += np.count_nonzero(clamped & ~alone)
                counts[4] += np.count_nonzero(alone)
                vel_out.append(_stored(_gather(carrier[a], taps, mutant, T), carrier[a], alone))
    return cell_out, vel_out, (counts & 0xffffffff).astype(np.uint32).view(np.int32), r

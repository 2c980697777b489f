"""The rule of ps_advect_fields_scheme with scheme 1 (include/polystokes.h "Advection schemes") restated in numpy on top of advection_ref.py:
the forward pass is that file's advect, sample for sample; the reverse trace, the corrected value, the limits and the fallback follow the
header line by line, fp64 from the fp32 inputs, no fused step.  Arrays are (z, y, x); a point p is the list (p_x, p_y, p_z).

MUTANTS names the near misses the shared cases must tell from the rule (test_advection_scheme_ref_cpu.py): advect(..., mutant=name)."""
import numpy as np

import advection_ref as ref

SEMI_LAGRANGIAN, MACCORMACK = 0, 1
LIMIT_NONE, LIMIT_CLAMP, LIMIT_REVERT = 0, 1, 2
MUTANTS = ("no_half",               # the whole error estimate added, not half of it
           "limits_at_p0",          # the limits from the sample's own neighbours instead of the taps at the departure point
           "limits_of_hat",         # the limits from the forward result instead of the source
           "bar_fp32",              # the reverse sample rounded to fp32 before it is used
           "hat_fp64",              # the forward result kept in fp64 instead of the fp32 grid it is
           "reverse_euler",         # the reverse trace at order 1 where order 2 is asked
           "reverse_from_p1",       # the reverse trace started at the departure point
           "no_fallback_on_clamp",  # a clamped sampler does not send the sample back to the forward value
           "clamp_is_revert",       # the clamp limiter reverting
           "limit_in_fallback")     # the limiter counted on the fallback samples too
SLOTS = 8                           # values the limiter changed on the four grids, then fallback samples of the four grids


def _trace_from(dims, carrier, p, r, order, T):
    """the departure rule started at the points p instead of the samples' own (the mutant reverse_from_p1): (q1, not finite)"""
    bad = np.zeros(p[0].shape, bool)
    U = ref._carrier_at(dims, carrier, p, None, T)
    if order == 2:
        half = T(0.5) * r
        qm, bad = ref._finite_or_alone([p[m] - half * U[m] for m in range(3)], bad, None, T)
        U = ref._carrier_at(dims, carrier, qm, None, T)
    return ref._finite_or_alone([p[m] - r * U[m] for m in range(3)], bad, None, T)


def _limits(F, taps, T):
    """lo, hi of the eight samples in the order x fastest, then y, then z; a NaN sample fails both comparisons"""
    (lx, hx, _), (ly, hy, _), (lz, hz, _) = taps
    lo = hi = None
    for z in (lz, hz):
        for y in (ly, hy):
            for x in (lx, hx):
                t = F[z, y, x].astype(T)
                if lo is None:
                    lo, hi = t.copy(), t.copy()
                else:
                    lo = np.where(t < lo, t, lo)
                    hi = np.where(t > hi, t, hi)
    return lo, hi


def _grid(dims, g, carrier, r, order, sources, limiter, mutant):
    """the outputs of grid g for its source fields: (outputs, forward clamped count, alone count, limited count, fallback count)"""
    T = np.float64
    p1, alone = ref.departure(dims, g, carrier, r, order)
    taps1, clamped1 = ref._taps(dims, g, p1, None, T)
    if mutant == "reverse_from_p1":
        q1, bad = _trace_from(dims, carrier, p1, -r, order, T)
    else:
        q1, bad = ref.departure(dims, g, carrier, -r, 1 if mutant == "reverse_euler" else order)       # from p0: negation is exact
    taps2, clamped2 = ref._taps(dims, g, q1, None, T)
    fallback = alone | bad
    if mutant != "no_fallback_on_clamp":
        fallback = fallback | clamped1 | clamped2
    if mutant == "limits_at_p0":
        d, o = ref.extents(dims, g), ref.offsets(g)
        k, j, i = np.meshgrid(np.arange(d[2]), np.arange(d[1]), np.arange(d[0]), indexing="ij")
        tapsL = ref._taps(dims, g, [i + T(o[0]), j + T(o[1]), k + T(o[2])], None, T)[0]
    else:
        tapsL = taps1
    outs, limited = [], 0
    for F in sources:
        sl = ref._gather(F, taps1, None, T)
        hat = ref._stored(sl, F, alone)                                        # the fp32 grid ps_advect_fields stores
        hat64 = np.where(alone, F.astype(T), sl) if mutant == "hat_fp64" else hat.astype(T)
        bar = ref._gather(hat64 if mutant == "hat_fp64" else hat, taps2, None, T)
        if mutant == "bar_fp32":
            bar = bar.astype(np.float32).astype(T)
        v = hat64 + (T(1.0) if mutant == "no_half" else T(0.5)) * (F.astype(T) - bar)
        if limiter != LIMIT_NONE:
            lo, hi = _limits(hat if mutant == "limits_of_hat" else F, tapsL, T)
            outside = (v < lo) | (v > hi)
            if limiter == LIMIT_CLAMP and mutant != "clamp_is_revert":
                v = np.where(v < lo, lo, np.where(v > hi, hi, v))
            else:
                v = np.where(outside, hat64, v)
            limited += np.count_nonzero(outside if mutant == "limit_in_fallback" else outside & ~fallback)
        outs.append(ref._stored(v, hat, fallback))
    return outs, np.count_nonzero(clamped1 & ~alone), np.count_nonzero(alone), limited, np.count_nonzero(fallback)


def advect(dims, dx, dt, order, carrier, cell_in=(), velocity=False, limiter=LIMIT_CLAMP, mutant=None):
    """(cell outputs, velocity outputs or None, counts int32[5], r, correction int32[8]) of a scheme 1 call; the first four as
    advection_ref.advect returns them for the forward pass"""
    carrier = [np.ascontiguousarray(c, np.float32) for c in carrier]
    r = np.float64(dt) / np.float64(dx)
    counts, corr = np.zeros(ref.SLOTS, np.int64), np.zeros(SLOTS, np.int64)
    cell_out, vel_out = [], None
    with np.errstate(all="ignore"):
        if len(cell_in):
            cell_out, counts[0], alone, corr[0], corr[4] = _grid(dims, 0, carrier, r, order, [np.ascontiguousarray(F, np.float32) for F in cell_in], limiter, mutant)
            counts[4] += alone
        if velocity:
            vel_out = []
            for a in range(3):
                out, counts[1 + a], alone, corr[1 + a], corr[5 + a] = _grid(dims, 1 + a, carrier, r, order, [carrier[a]], limiter, mutant)
                counts[4] += alone
                vel_out.append(out[0])
    wrap = lambda n: (n & 0xffffffff).astype(np.uint32).view(np.int32)
    return cell_out, vel_out, wrap(counts), r, wrap(corr)

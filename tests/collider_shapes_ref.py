"""The rule of ps_place_colliders (include/polystokes.h) restated in numpy, vectorised over cells with a loop over colliders.  Arrays are
(z, y, x) as everywhere in the tests: axis a of the rule is numpy axis 2 - a, of the world grid and of a volume alike.  All arithmetic is
fp64 from the fp32 / fp64 inputs, elementwise (numpy fuses nothing), in the order the header writes it, so the device's grids are expected
byte for byte.

MUTANTS are near misses of the rule, switched on by name; test_collider_shapes_ref_cpu.py shows that the cases tell each from the rule."""
import numpy as np

REACH = 4.0     # PS_COLLIDER_SHAPE_REACH
# rotation: R instead of its transpose; no_half: s_a without the - 0.5 (samples on the volume's grid lines); tie_new: D_k >= D_best
MUTANTS = ("rotation", "no_half", "tie_new")


def place(collision, ids, shapes, poses, orig, dx, negate=1, mutant=None):
    """collision: fp32 (nz, ny, nx); ids: int32 cell field or None (then -1 everywhere); shapes: a sequence of (sdf fp32 (n2, n1, n0), h,
    o[3]); poses: (count, 12) fp64.  Returns (collision fp32, ids int32, int32 counters of count + 2)."""
    col = np.asarray(collision, np.float32)
    poses = np.asarray(poses, np.float64).reshape(-1, 12)
    count = len(shapes)
    assert poses.shape[0] == count
    dx = float(dx)
    idx = np.indices(col.shape)
    r = [float(orig[m]) + (idx[2 - m].astype(np.float64) + 0.5) * dx for m in range(3)]
    base = col.astype(np.float64)
    best = -base if negate else base.copy()
    kbest = np.full(col.shape, -1, np.int64)
    skipped = 0
    for k in range(count):
        if not np.isfinite(poses[k]).all():
            skipped += 1
            continue
        sdf, h, o = shapes[k]
        v = np.asarray(sdf, np.float32).astype(np.float64)
        h = float(h)
        n = v.shape[::-1]
        R, t = poses[k, :9].reshape(3, 3), poses[k, 9:]
        with np.errstate(invalid="ignore", over="ignore"):
            d = [r[m] - t[m] for m in range(3)]
            E = (REACH * dx) / h
            s, part = [], np.ones(col.shape, bool)
            for a in range(3):
                if mutant == "rotation":
                    q = (R[a][0] * d[0] + R[a][1] * d[1]) + R[a][2] * d[2]
                else:
                    q = (R[0][a] * d[0] + R[1][a] * d[1]) + R[2][a] * d[2]
                sa = (q - float(o[a])) / h if mutant == "no_half" else (q - float(o[a])) / h - 0.5
                part &= (sa >= -E) & (sa <= float(n[a] - 1) + E)
                s.append(sa)
            i, f, out = [], [], []
            for a in range(3):
                sa = np.where(part, s[a], 0.0)          # (elsewhere anything: an infinity or a NaN must not reach the integer cast)
                ca = np.minimum(np.maximum(sa, 0.0), float(n[a] - 1))
                ia = np.minimum(np.floor(ca).astype(np.int64), n[a] - 2)
                i.append(ia)
                f.append(ca - ia.astype(np.float64))
                out.append((sa - ca) * h)
            V = lambda dz, dy, dx_: v[i[2] + dz, i[1] + dy, i[0] + dx_]
            x00 = V(0, 0, 0) + (V(0, 0, 1) - V(0, 0, 0)) * f[0]
            x10 = V(0, 1, 0) + (V(0, 1, 1) - V(0, 1, 0)) * f[0]
            x01 = V(1, 0, 0) + (V(1, 0, 1) - V(1, 0, 0)) * f[0]
            x11 = V(1, 1, 0) + (V(1, 1, 1) - V(1, 1, 0)) * f[0]
            y0 = x00 + (x10 - x00) * f[1]
            y1 = x01 + (x11 - x01) * f[1]
            val = y0 + (y1 - y0) * f[2]
            dist = np.sqrt((out[0] * out[0] + out[1] * out[1]) + out[2] * out[2])
            Dk = (-val if negate else val) - dist
            wins = part & ((Dk >= best) if mutant == "tie_new" else (Dk > best))
        best = np.where(wins, Dk, best)
        kbest = np.where(wins, k, kbest)
    won = kbest >= 0
    with np.errstate(over="ignore"):
        new = (-best if negate else best).astype(np.float32)
    col_out = np.where(won, new, col).astype(np.float32)
    ids0 = np.full(col.shape, -1, np.int32) if ids is None else np.asarray(ids, np.int32)
    ids_out = np.where(won, kbest, ids0).astype(np.int32)
    counters = np.zeros(count + 2, np.int64)
    counters[:count] = np.bincount(kbest[won], minlength=count)
    counters[count] = int((~won).sum())
    counters[count + 1] = skipped
    return col_out, ids_out, counters.astype(np.int32)

"""Plain numpy / Python restatement of the air pockets of ps_label_air_pockets (include/polystokes.h): a union-find over the links, no
device code.  Arrays are numpy (z, y, x) — x fastest — as polystokes_amd.Solver.array returns them after a reshape.

pockets(lw, fw, fwx, fwy, fwz, dx) -> dict(ids, units, cells, open, volume)
  lw, fw: "centerLiquidWeights", "centerFluidWeights" (nz, ny, nx); fwx / fwy / fwz: "faceX/Y/ZFluidWeights".
mutant (tests only): "closed_faces_link" links two core cells through a face with fwF = 0; "number_by_size" numbers the pockets by
falling cell count instead of by their smallest cell index."""
import numpy as np

UNIT = 1048576.0
# -x, +x, -y, +y, -z, +z as (numpy axis, sign)
DIRECTIONS = ((2, -1), (2, +1), (1, -1), (1, +1), (0, -1), (0, +1))


def _shift(a, axis, sgn, fill):
    """out[c] = a[c + sgn e_axis], `fill` where that neighbour lies outside the grid"""
    out = np.full_like(a, fill)
    src, dst = [slice(None)] * 3, [slice(None)] * 3
    if sgn > 0:
        src[axis], dst[axis] = slice(1, None), slice(0, -1)
    else:
        src[axis], dst[axis] = slice(0, -1), slice(1, None)
    out[tuple(dst)] = a[tuple(src)]
    return out


def _face_towards(fwF, axis, sgn):
    """the weight of the face between every cell and its neighbour at sgn e_axis (the face grid has one more sample along its axis)"""
    n = fwF.shape[axis] - 1
    sl = [slice(None)] * 3
    sl[axis] = slice(1, n + 1) if sgn > 0 else slice(0, n)
    return fwF[tuple(sl)]


def _find(parent, i):
    r = i
    while parent[r] != r:
        r = parent[r]
    while parent[i] != r:
        parent[i], i = r, parent[i]
    return r


def pockets(lw, fw, fwx, fwy, fwz, dx, mutant=None):
    lw, fw = np.asarray(lw, np.float32), np.asarray(fw, np.float32)
    faces = {2: np.asarray(fwx, np.float32), 1: np.asarray(fwy, np.float32), 0: np.asarray(fwz, np.float32)}
    shape = lw.shape
    n = lw.size
    core = (fw > 0) & (lw <= np.float32(0.5))
    index = np.arange(n, dtype=np.int64).reshape(shape)
    # union-find over the links; the root of a set is its smallest cell index
    parent = list(range(n))
    for axis in (2, 1, 0):
        open_face = _face_towards(faces[axis], axis, +1) > 0
        if mutant == "closed_faces_link":
            open_face = np.ones_like(open_face)
        linked = core & _shift(core, axis, +1, False) & open_face
        a = index[linked]
        b = _shift(index, axis, +1, -1)[linked]
        for p, q in zip(a.tolist(), b.tolist()):
            rp, rq = _find(parent, p), _find(parent, q)
            if rp != rq:
                parent[max(rp, rq)] = min(rp, rq)
    flat_core = core.ravel()
    root = np.full(n, -1, np.int64)
    for c in np.flatnonzero(flat_core).tolist():
        root[c] = _find(parent, c)
    roots = np.unique(root[flat_core])                      # rising: numbering by the smallest cell index
    if mutant == "number_by_size" and roots.size:
        size = np.array([(root == r).sum() for r in roots])
        roots = roots[np.argsort(-size, kind="stable")]
    number = {int(r): k for k, r in enumerate(roots.tolist())}
    K = len(number)
    ids = np.full(n, -1, np.int32)
    for c in np.flatnonzero(flat_core).tolist():
        ids[c] = number[int(root[c])]
    ids = ids.reshape(shape)
    # skin cells: the core neighbour with the smallest lw across a face with fwF > 0, the first of a tie in direction order
    core_ids = ids.copy()
    candidate = (~core) & (fw > 0) & (lw < np.float32(1.0))
    best_lw = np.full(shape, np.inf, np.float64)
    best_id = np.full(shape, -1, np.int32)
    for axis, sgn in DIRECTIONS:
        ok = candidate & _shift(core, axis, sgn, False) & (_face_towards(faces[axis], axis, sgn) > 0)
        nlw = _shift(lw, axis, sgn, np.float32(0)).astype(np.float64)
        take = ok & (nlw < best_lw)
        best_lw[take] = nlw[take]
        best_id[take] = _shift(core_ids, axis, sgn, -1)[take]
    skin = candidate & (best_id >= 0)
    ids[skin] = best_id[skin]
    # sums
    u = np.rint(fw.astype(np.float64) * (1.0 - lw.astype(np.float64)) * UNIT).astype(np.int64)
    units, cells, opened = np.zeros(K, np.int64), np.zeros(K, np.int32), np.zeros(K, np.int32)
    has = ids >= 0
    np.add.at(units, ids[has], u[has])
    np.add.at(cells, ids[core], 1)
    border = np.zeros(shape, bool)
    border[0], border[-1], border[:, 0], border[:, -1], border[:, :, 0], border[:, :, -1] = True, True, True, True, True, True
    opened[np.unique(ids[core & border])] = 1
    dx = float(dx)
    volume = (units.astype(np.float64) * (1.0 / UNIT)) * (dx * dx * dx)
    return {"ids": ids, "units": units, "cells": cells, "open": opened, "volume": volume}


def pressure_field(ids, p):
    """the cell field ps_set_air_pocket_pressures writes: (float)p[id] where id >= 0, 0 elsewhere"""
    p = np.asarray(p, np.float64)
    out = np.zeros(ids.shape, np.float32)
    has = ids >= 0
    out[has] = p[ids[has]].astype(np.float32)
    return out

"""Shared by tests/test_gpu_extrapolation.py and its child processes: the scenes of the velocity-extrapolation tests, one step with a given
setting, and the digest the child processes print.

As a script (child process, the switches of the library are read once per process):
    extrapolation_cases.py step <scene> <layers>                       one step on a fresh context; prints "DIGEST <sha256>" of digest()
    extrapolation_cases.py slab <layers> <rank> <base_port> <out.npz>  rank <rank> of a two-rank slab pair of cavity(32, tile=8) over TCP"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

LAYER_ARRAYS = ("extrapolationLayerX", "extrapolationLayerY", "extrapolationLayerZ")


def scene(name):
    """blob0: non-cubic and ragged (24 x 20 x 28: the three face grids differ in every extent); droplet24: droplet(24) carrying a rigid
    rotation (the scene's own velocity is zero everywhere, which no extrapolation could get wrong); sliding32: a box on a floor, saturates
    within 12 layers; cavity32: no invalid face; spheres32: a solve long enough to interrupt."""
    from polystokes_amd import _abi as abi
    from polystokes_amd import scenes
    if name == "blob0":
        return scenes.blob(seed=0)
    if name == "droplet24":
        from helpers import rigid_rotation_scene
        sc, p, _ = rigid_rotation_scene(24)
        return sc, p
    if name == "sliding32":
        return scenes.sliding_block(32)
    if name == "cavity32":
        return scenes.cavity(32)
    if name == "cavity32t8":
        return scenes.cavity(32, tile=8)
    if name == "spheres32":
        sc, p = scenes.spheres(32, tile=8)
        p.preconditioner, p.tolerance, p.maxSolverIterations = abi.PRE_DIAGONAL, 1e-8, 20000
        return sc, p
    raise KeyError(name)


def outcome(s, rc):
    """what a host-boundary step left: rc, iterations, x, vel, valid, and the extrapolation's arrays (layer / counts: None when not registered)"""
    out = {"rc": int(rc), "iterations": int(s.stats.solveData[1]), "x": s.array("solutionVector").tobytes(),
           "vel": [np.array(v, copy=True) for v in s.vel], "valid": [np.array(v, copy=True) for v in s.valid],
           "used": int(s.array("velocityExtrapolation")[0]), "layer": None, "counts": None}
    try:
        out["layer"] = [s.array(n).reshape(s.vel[a].shape) for a, n in enumerate(LAYER_ARRAYS)]
        out["counts"] = s.array("extrapolationCounts")
    except KeyError:
        pass
    return out


def step(s, sc, p, layers=None):
    """polystokes_step on `s`, after ps_set_velocity_extrapolation(layers) unless layers is None (a context that never made the call)"""
    from polystokes_amd import _abi as abi
    if layers is not None:
        assert s.set_velocity_extrapolation(layers) == abi.SUCCESS, s.last_error()
    return outcome(s, s.step(sc, p))


def fresh(name, layers=None):
    import polystokes_amd
    sc, p = scene(name)
    s = polystokes_amd.Solver(0)
    try:
        return step(s, sc, p, layers)
    finally:
        s.close()


def digest(vel, valid, layer, counts, used):
    h = hashlib.sha256()
    for group in (vel, valid, layer):
        for a in group:
            h.update(np.ascontiguousarray(a).tobytes())
    h.update(np.ascontiguousarray(counts, dtype=np.int32).tobytes())
    h.update(b"%d" % int(used))
    return h.hexdigest()


def _child_step(name, layers):
    got = fresh(name, layers)
    assert got["layer"] is not None, "no layer arrays"
    print("DIGEST", digest(got["vel"], got["valid"], got["layer"], got["counts"], got["used"]))


def _child_slab(layers, rank, port, out):
    import polystokes_amd
    from polystokes_amd import partition
    sc, p = scene("cavity32t8")
    sl = partition.make_slab(sc.nz, 2, rank, p.tileSize)
    s = polystokes_amd.Solver(0)
    if layers >= 0:
        assert s.set_velocity_extrapolation(layers) == 1
    s.upload(partition.local_scene(sc, sl), p)
    s.set_slab(sl)
    s.comm_init_tcp(rank, 2, "127.0.0.1", port)
    rc = s.step_device()
    lv, lval = s.download()
    res = {"rc": rc, "iterations": int(s.stats.solveData[1]), "used": int(s.array("velocityExtrapolation")[0]),
           "has_layer": int(s.L.ps_query_array(s.h, b"extrapolationLayerX", None) >= 0)}
    for a in range(3):
        res["vel%d" % a], res["valid%d" % a] = lv[a], lval[a]
    np.savez(out, **res)
    s.close()


if __name__ == "__main__":
    if sys.argv[1] == "step":
        _child_step(sys.argv[2], int(sys.argv[3]))
    else:
        _child_slab(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])

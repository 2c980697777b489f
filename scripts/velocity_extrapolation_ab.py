#!/usr/bin/env python3
"""The write-back stage (stats.stage_ms[PS_STAGE_WRITEBACK]) with ps_set_velocity_extrapolation at 0 / 4 / 16 / 64 layers on the 256^3
cavity and coil, in ONE process, the configurations alternating step by step:
  parent   the library of another checkout (--parent DIR: that tree's polystokes_amd/ with its built library), which has no such call
  new      this tree's library
  variant  another build of this tree's library (--variant LIB, e.g. a different sweep kernel), through this tree's Python layer
and the box's device-to-device copy rate (1 GiB, read + write counted).  The solve is cut at 25 iterations (NOCONVERGE is kept, so the
write-back runs as after a full solve; what it costs does not depend on how far the solve got).
usage: velocity_extrapolation_ab.py [--parent DIR] [--variant LIB] [--res 256] [--rounds 5] [--out FILE.json]"""
import argparse
import importlib
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None)
ap.add_argument("--variant", default=None)
ap.add_argument("--res", type=int, default=256)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
WRITEBACK = 10      # PS_STAGE_WRITEBACK


def load_pkg(name, path, lib=None):
    """the Python layer at `path` as a package of its own name (its ctypes types stay its own), bound to `lib` (None: the one beside it)"""
    if lib:
        os.environ["PS_LIB"] = lib
    else:
        os.environ.pop("PS_LIB", None)
    spec = importlib.util.spec_from_file_location(name, os.path.join(path, "__init__.py"), submodule_search_locations=[path])
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    importlib.import_module(name + ".scenes")
    os.environ.pop("PS_LIB", None)
    return m


def copy_rate(pkg):
    _hip = importlib.import_module(pkg.__name__ + "._hip")
    n = 256 * 1024 * 1024          # floats: 1 GiB
    a, b = _hip.DeviceBuffer(n), _hip.DeviceBuffer(n)
    st = _hip.Stream()
    best = 1e9
    for rep in range(6):
        t0 = time.perf_counter()
        for _ in range(4):
            _hip.memcpy_async(b.ptr, a.ptr, a.nbytes, _hip.D2D, st.cuda_stream)
        st.synchronize()
        if rep:
            best = min(best, (time.perf_counter() - t0) / 4)
    a.close(); b.close(); st.close()
    return {"copy_1GiB_ms": best * 1e3, "copy_GBps_read_plus_write": 2 * n * 4 / best / 1e9}


pk = {"new": load_pkg("ps_new", os.path.join(ROOT, "polystokes_amd"))}
configs = [("new", 0), ("new", 4), ("new", 16), ("new", 64)]
if args.parent:
    pk["parent"] = load_pkg("ps_parent", os.path.join(args.parent, "polystokes_amd"))
    configs.insert(0, ("parent", None))
if args.variant:
    pk["variant"] = load_pkg("ps_variant", os.path.join(ROOT, "polystokes_amd"), os.path.abspath(args.variant))
    configs += [("variant", 4), ("variant", 16), ("variant", 64)]
res = {"libraries": {k: m.LIB_PATH for k, m in pk.items()}, "copy": copy_rate(pk["new"])}
print(json.dumps(res), flush=True)
for scene in ("cavity", "coil"):
    solvers, counts = {}, {}
    for k, m in pk.items():
        sc, p = getattr(m.scenes, scene)(args.res)
        p.preconditioner = 5            # Jacobi
        p.maxSolverIterations = 25
        s = m.Solver(0)
        s.upload(sc, p)
        solvers[k] = s
        faces = (sc.nx + 1) * sc.ny * sc.nz + sc.nx * (sc.ny + 1) * sc.nz + sc.nx * sc.ny * (sc.nz + 1)
    times = {c: [] for c in configs}
    for rep in range(args.rounds + 1):  # the first round warms up
        for c in configs:
            s = solvers[c[0]]
            if c[1] is not None:
                assert s.set_velocity_extrapolation(c[1]) == 1
            s.step_device()
            if rep:
                times[c].append(float(s.stats.stage_ms[WRITEBACK]))
            if c[1]:
                counts[c] = [int(v) for v in s.array("extrapolationCounts")]
    r = {"faces": faces}
    for c in configs:
        r["%s_L%s" % c] = {"median_ms": float(np.median(times[c])), "min_ms": min(times[c]), "max_ms": max(times[c])}
    for c, v in counts.items():
        r["assigned_%s_L%s" % c] = sum(v)
    res[scene] = r
    print(scene, json.dumps(r), flush=True)
    for s in solvers.values():
        s.close()
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)

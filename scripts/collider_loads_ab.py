#!/usr/bin/env python3
"""What ps_set_collider_loads adds to a step: the write-back stage (stats.stage_ms[PS_STAGE_WRITEBACK]) and the whole step on spheres at
--res^3, in ONE process, the configurations alternating step by step:
  parent   the library of another checkout (--parent DIR: that tree's polystokes_amd/ with its built library), which has no such call
  off      this tree's library, a context that never makes the call
  on       this tree's library, a context with count = 8, the nearest-sphere id field, the sphere centres as pivots
Every configuration has a context of its own, set up once; the order of the three rotates from round to round.
The solve is cut at 25 iterations (NOCONVERGE is kept, so the loads run as after a full solve; what they cost does not depend on how far
the solve got).  Prints the bytes the pass must move: x once, seven weight grids, one id grid.
usage: collider_loads_ab.py [--parent DIR] [--res 256] [--rounds 5] [--create-reversed] [--out FILE.json]"""
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
ap.add_argument("--res", type=int, default=256)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--create-reversed", action="store_true", help="create the contexts in the opposite order (where a context's buffers land is part of its speed)")
args = ap.parse_args()
WRITEBACK = 10      # PS_STAGE_WRITEBACK


def load_pkg(name, path):
    """the Python layer at `path` as a package of its own name (its ctypes types stay its own), bound to the library beside it"""
    os.environ.pop("PS_LIB", None)
    spec = importlib.util.spec_from_file_location(name, os.path.join(path, "__init__.py"), submodule_search_locations=[path])
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    importlib.import_module(name + ".scenes")
    return m


def sphere_ids(sc, nspheres=8, seed=12345):
    """the nearest sphere of scenes.spheres per cell (the same draws in the same order), and the centres"""
    rng = np.random.RandomState(seed)
    k, j, i = np.meshgrid(np.arange(sc.nz, dtype=np.float32), np.arange(sc.ny, dtype=np.float32), np.arange(sc.nx, dtype=np.float32),
                          indexing="ij", sparse=True)
    x, y, z = (i + 0.5) * sc.dx, (j + 0.5) * sc.dx, (k + 0.5) * sc.dx
    best, ids, cen = None, None, []
    for q in range(nspheres):
        c = rng.uniform(0.2, 0.8, 3)
        c[1] = rng.uniform(0.25, 0.55)
        rad = rng.uniform(0.06, 0.11)
        rng.uniform(-1.0, 1.0, 3)
        cen.append(c)
        d = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - rad
        if best is None:
            best, ids = d, np.zeros(d.shape, np.int32)
        else:
            ids[d < best] = q
            best = np.minimum(best, d)
    return ids, np.array(cen)


pk = {"new": load_pkg("ps_new", os.path.join(ROOT, "polystokes_amd"))}
configs = [("new", 0), ("new", 8)]
if args.parent:
    pk["parent"] = load_pkg("ps_parent", os.path.join(args.parent, "polystokes_amd"))
    configs.insert(0, ("parent", None))
solvers = {}
for c in (configs[::-1] if args.create_reversed else configs):
    m = pk[c[0]]
    sc, p = m.scenes.spheres(args.res)
    p.preconditioner = 5            # Jacobi
    p.maxSolverIterations = 25
    s = m.Solver(0)
    s.upload(sc, p)
    if c[1]:
        ids, centres = sphere_ids(sc)
        assert s.set_collider_loads(c[1], centres) == 1
        assert s.upload_collider_ids(ids) == 1
    solvers[c] = (s, sc, p)
n = args.res
res = {"libraries": {k: m.LIB_PATH for k, m in pk.items()}, "res": n}
wb = {c: [] for c in configs}
total = {c: [] for c in configs}
for rep in range(args.rounds + 1):      # the first round warms up
    for q in range(len(configs)):
        c = configs[(q + rep) % len(configs)]
        s, sc, p = solvers[c]
        t0 = time.perf_counter()
        s.step_device()                 # (ends with the stream synchronised)
        t1 = time.perf_counter()
        if rep:
            wb[c].append(float(s.stats.stage_ms[WRITEBACK]))
            total[c].append((t1 - t0) * 1e3)
s = solvers[("new", 8)][0]
nsys = int(s.stats.dimData[21])
grids = n ** 3 + 3 * (n + 1) * n * n + 3 * (n + 1) * (n + 1) * n         # centre liquid, three face fluid, three edge liquid weights
maps = 4 * n ** 3 + 3 * (n + 1) * (n + 1) * n                            # the seven index maps (read to find the DOFs)
res["bytes"] = {"x": 8 * nsys, "weights_7_grids": 4 * grids, "ids": 4 * n ** 3, "index_maps": 4 * maps}
res["bytes"]["must_move"] = res["bytes"]["x"] + res["bytes"]["weights_7_grids"] + res["bytes"]["ids"]
res["terms"] = [int(v) for v in s.array("colliderLoadTerms")]
res["force"] = s.array("colliderForce").reshape(-1, 3).tolist()
for c in configs:
    res["%s_count%s" % c] = {"writeback_median_ms": float(np.median(wb[c])), "writeback_min_ms": min(wb[c]), "writeback_max_ms": max(wb[c]),
                             "step_median_ms": float(np.median(total[c])), "step_min_ms": min(total[c]), "step_max_ms": max(total[c])}
print(json.dumps(res, indent=1), flush=True)
for s, _, _ in solvers.values():
    s.close()
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)

#!/usr/bin/env python3
"""Host boundary against device boundary on one box, in ONE process: one context per scene, and after a warm-up its steps alternate between
  host      polystokes_step (host arrays in, host arrays out: the parent path)
  resident  ps_step_device on the fields of the last upload (no boundary at all: the floor)
  dev0      ps_step_device_fields on device arrays, x fastest (k_fields_copy in and out)
  dev1      ps_step_device_fields on device arrays, z fastest (k_fields_swap_xz in and out)
each timed by a host clock around a call that ends synchronised (the device modes synchronise the caller's stream).  Then the emit alone
(ps_download_fields_device, both layouts) beside a hipMemcpy device-to-device of the same bytes, all three timed the same way.
Prints (and with --out appends) a markdown section.  Jacobi, tolerance 1e-3.
usage: device_fields_ab.py [--cases coil:128,coil:256,cavity:256] [--rounds 3] [--out FILE]
Under rocprofv3 --kernel-trace --stats run it with --rounds 1: the k_fields_* rows are the ingest and emit kernel times."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="coil:128,coil:256,cavity:256")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

import numpy as np
import polystokes_amd
from polystokes_amd import scenes, _abi as abi, _hip

lines = []
def say(s=""):
    print(s, flush=True)
    lines.append(s)


def sync():
    _hip.check(_hip.rt().hipStreamSynchronize(None), "hipStreamSynchronize")


def timed(fn):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


MODES = ("host", "resident", "dev0", "dev1")
say("### host boundary against device boundary, Jacobi, tol 1e-3, %d rounds alternating in one process" % args.rounds)
say()
say("| scene | mode | ms/step (each round) | best | iterations | bytes in + out per step (read + written) |")
say("|---|---|---|---|---|---|")
emit = []
for case in args.cases.split(","):
    name, res = case.split(":")
    res = int(res)
    sc, p = {"cavity": scenes.cavity, "coil": scenes.coil}[name](res)
    p.preconditioner, p.tolerance = abi.PRE_DIAGONAL, 1e-3
    sh = abi.grid_shapes(sc.nx, sc.ny, sc.nz)
    n_in = 4 * (3 * int(np.prod(sh["center"])) + 2 * sum(int(np.prod(sh["face" + a])) for a in "XYZ"))
    n_out = 4 * 2 * sum(int(np.prod(sh["face" + a])) for a in "XYZ")
    s = polystokes_amd.Solver(0)
    dev = {0: polystokes_amd.device_scene(sc, 0), 1: polystokes_amd.device_scene(sc, 1)}
    outs = {l: ([_hip.DeviceBuffer(b.count) for b in dev[l].vel], [_hip.DeviceBuffer(b.count) for b in dev[l].vel]) for l in (0, 1)}
    run = {
        "host": lambda: s.step(sc, p),
        "resident": lambda: s.step_device(),
        "dev0": lambda: s.step_device_fields(p, dev[0], 0, out=outs[0]),
        "dev1": lambda: s.step_device_fields(p, dev[1], 1, out=outs[1]),
    }
    for m in MODES:
        run[m]()                                              # warm-up: code objects, buffers
    rec = {m: [] for m in MODES}
    its = {}
    for _ in range(args.rounds):
        for m in MODES:
            rec[m].append(timed(run[m]))
            its[m] = int(s.stats.solveData[1])
    for m in MODES:
        by = {"host": n_in + n_out, "resident": 0}.get(m, 2 * (n_in + n_out))
        say("| %s %d | %s | %s | %.1f | %d | %.1f MB |" % (name, res, m, " / ".join("%.1f" % v for v in rec[m]), min(rec[m]), its[m], by / 1e6))
    # the emit alone, and a device-to-device copy of the same bytes
    src, dst = _hip.DeviceBuffer(n_out // 4), _hip.DeviceBuffer(n_out // 4)
    e = {"emit0": [], "emit1": [], "copy": []}
    for _ in range(args.rounds + 1):
        e["emit0"].append(timed(lambda: s.download_device(0, out=outs[0])))
        e["emit1"].append(timed(lambda: s.download_device(1, out=outs[1])))
        e["copy"].append(timed(lambda: _hip.memcpy(dst.ptr, src.ptr, n_out, _hip.D2D)))
    emit.append((name, res, n_out, {k: min(v[1:]) for k, v in e.items()}))
    print("RAW " + json.dumps({"scene": name, "res": res, "rec": rec, "emit": e}), flush=True)
    s.close()
    for b in [src, dst] + [x for l in (0, 1) for x in outs[l][0] + outs[l][1]]:
        b.close()
    del dev
say()
say("| scene | emit bytes (read + written) | k_fields_copy call ms | k_fields_swap_xz call ms | hipMemcpy DtoD ms | swap GB/s | copy GB/s | swap / copy rate |")
say("|---|---|---|---|---|---|---|---|")
for name, res, n_out, t in emit:
    gb = 2 * n_out / 1e9
    say("| %s %d | %.1f MB | %.3f | %.3f | %.3f | %.0f | %.0f | %.2f |" % (name, res, 2 * n_out / 1e6, t["emit0"], t["emit1"], t["copy"], gb / (t["emit1"] * 1e-3),
                                                                    gb / (t["copy"] * 1e-3), t["copy"] / t["emit1"]))
say()
say("(call ms: host clock around the call and a synchronisation of the caller's stream, best of %d: launch and event overhead included)" % args.rounds)
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")

#!/usr/bin/env python3
"""fp64 against mixed-precision PCG (ps_set_solve_precision) on one box, in ONE process: two contexts hold the same scene, one per mode, and
their steps alternate (as scripts/env_ab.py alternates children), so both modes see the same box in the same minute.  Jacobi, tol 1e-3
unless asked otherwise.  Prints (and with --out appends) a markdown section: ms/step, solve ms, iterations, passes, ms per iteration of each
mode, and the box's device-to-device copy rate (a torch copy in a child process, before the solves).
usage: mixed_precision_ab.py [--res 256] [--scenes cavity,coil,spheres] [--rounds 3] [--tol 1e-3] [--precond jacobi|identity] [--modes 0,1] [--out FILE]
Under rocprofv3 --kernel-trace --stats run it with --modes 1 --rounds 1 --no-copy: the kernel table of a mixed run."""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, default=256)
ap.add_argument("--scenes", default="cavity,coil,spheres")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--tol", type=float, default=1e-3)
ap.add_argument("--precond", default="jacobi")
ap.add_argument("--modes", default="0,1")
ap.add_argument("--out", default=None)
ap.add_argument("--no-copy", action="store_true")
args = ap.parse_args()

_COPY = ("import torch\nn = 1 << 27\na = torch.empty(n, dtype=torch.float64, device='cuda').fill_(1.0); b = torch.empty_like(a)\n"
         "for _ in range(3): b.copy_(a)\ntorch.cuda.synchronize()\ne0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)\n"
         "e0.record()\nfor _ in range(20): b.copy_(a)\ne1.record(); torch.cuda.synchronize()\nprint('COPY', 2.0 * n * 8 * 20 / (e0.elapsed_time(e1) * 1e-3) / 1e9)\n")


def copy_rate():
    pr = subprocess.run([sys.executable, "-c", _COPY], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    line = [l for l in pr.stdout.splitlines() if l.startswith("COPY ")]
    return float(line[0].split()[1]) if line else float("nan")


lines = []
def say(s=""):
    print(s, flush=True)
    lines.append(s)


rate = float("nan") if args.no_copy else copy_rate()
import numpy as np
import polystokes_amd
from polystokes_amd import scenes, _abi as abi

modes = [int(m) for m in args.modes.split(",")]
pre = {"jacobi": abi.PRE_DIAGONAL, "identity": abi.PRE_IDENTITY}[args.precond]
say("### %d^3, %s, tol %g, %d rounds alternating; device-to-device copy %.0f GB/s" % (args.res, args.precond, args.tol, args.rounds, rate))
say()
say("| scene | mode | ms/step (each round) | solve ms | iterations | passes | ms per iteration | used | fused step |")
say("|---|---|---|---|---|---|---|---|---|")
for name in args.scenes.split(","):
    make = {"cavity": lambda: scenes.cavity(args.res), "coil": lambda: scenes.coil(args.res), "spheres": lambda: scenes.spheres(args.res)}[name]
    sc, p = make()
    p.preconditioner, p.tolerance = pre, args.tol
    ctx = {}
    for m in modes:
        s = polystokes_amd.Solver(0)
        assert s.set_solve_precision(m) == abi.SUCCESS
        s.upload(sc, p)
        s.step_device()                                       # warm-up: code objects, buffers
        ctx[m] = s
    rec = {m: [] for m in modes}
    for _ in range(args.rounds):
        for m in modes:
            s = ctx[m]
            t0 = time.time()
            rc = s.step_device()                              # ends with the stream synchronised
            ms = (time.time() - t0) * 1e3
            used = int(s.array("solvePrecisionUsed")[0])
            rec[m].append(dict(ms=ms, solve=float(s.stats.stage_ms[8]), it=int(s.stats.solveData[1]), rc=int(rc), used=used,
                               passes=[int(v) for v in s.array("solvePassIterations")] if used else [], fused=int(s.array("fusedStep")[0]),
                               err=float(s.stats.solveData[0])))
    for m in modes:
        r = rec[m]
        best = min(r, key=lambda d: d["ms"])
        say("| %s | %s | %s | %.1f | %d | %s | %.4f | %d | %d |" % (name, "mixed" if m else "fp64", " / ".join("%.1f" % d["ms"] for d in r), best["solve"], best["it"],
                                                                 best["passes"] or "-", best["solve"] / max(best["it"], 1), best["used"], best["fused"]))
    if len(modes) == 2:
        a, b = min(d["ms"] for d in rec[0]), min(d["ms"] for d in rec[1])
        say("| %s | mixed / fp64 | %.3f of the step, %.3f of the solve per iteration | | | | | | |" % (
            name, b / a, (min(rec[1], key=lambda d: d["ms"])["solve"] / max(rec[1][0]["it"], 1)) / (min(rec[0], key=lambda d: d["ms"])["solve"] / max(rec[0][0]["it"], 1))))
    print("RAW " + json.dumps({"scene": name, "res": args.res, "rec": rec}), flush=True)
    for s in ctx.values():
        s.close()
say()
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")

"""Warm start against cold start over time sequences (ps_set_warm_start, DESIGN.md "Warm start").

Two contexts run side by side, one in mode PS_WARM_NONE (cold) and one in PS_WARM_PREVIOUS_STEP (warm).  Step k of a sequence feeds BOTH
the same input: the cold context's output velocity of step k-1 (and, for the spheres scene, the spheres advanced to t = k dt), so the two
columns of a row solve the same system and differ only in x0.  A step is timed as bench.py times it: wall clock around ps_step_device
(which returns with the stream synchronised); uploads and downloads are outside the timed region.

    python scripts/warm_start_sequence.py [--cases cavity128,cavity256,spheres256,coil256] [--steps 10] [--precond jacobi] [--out FILE]

Prints one JSON line per step and one summary line per case; --out also writes them to FILE.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import polystokes_amd  # noqa: E402
from polystokes_amd import _abi as abi  # noqa: E402
from polystokes_amd import scenes  # noqa: E402

PRECONDS = {"identity": abi.PRE_IDENTITY, "jacobi": abi.PRE_DIAGONAL, "chebyshev": abi.PRE_CHEBYSHEV, "chebyshev_f32": abi.PRE_CHEBYSHEV_F32}


def make(case, k):
    """the scene of step k (geometry only; the velocity is replaced by the previous step's output from step 1 on)"""
    n = int("".join(ch for ch in case if ch.isdigit()))
    if case.startswith("cavity"):
        return scenes.cavity(n)
    if case.startswith("spheres"):
        return scenes.spheres(n, t=k / 48.0)          # (the scene's dt)
    if case.startswith("coil"):
        return scenes.coil(n)
    raise ValueError(case)


def run_case(case, steps, precond, emit):
    cold, warm = polystokes_amd.Solver(0), polystokes_amd.Solver(0)
    warm.set_warm_start(abi.WARM_PREVIOUS_STEP)
    vel = None
    rows = []
    for k in range(steps):
        sc, p = make(case, k)
        p.preconditioner = precond
        if vel is not None:
            for a in range(3):
                sc.vel[a][...] = vel[a]
        rec = {"case": case, "step": k}
        for name, s in (("cold", cold), ("warm", warm)):
            s.upload(sc, p)
            t0 = time.perf_counter()
            rc = s.step_device()
            ms = (time.perf_counter() - t0) * 1e3
            rec[name] = {"rc": rc, "iterations": int(s.stats.solveData[1]), "ms": round(ms, 2),
                         "solve_ms": round(s.stats.stage_ms[abi.STAGE_NAMES.index("solve")], 2),
                         "warm_used": int(s.array("warmStartUsed")[0])}
        vel = [v.copy() for v in cold.download()[0]]
        w = warm.download()[0]
        rec["warm_vs_cold_vel_rel"] = float(max(np.abs(w[a] - vel[a]).max() for a in range(3)) / max(max(np.abs(v).max() for v in vel), 1e-30))
        rows.append(rec)
        emit(rec)
    cold.close()
    warm.close()
    later = rows[1:]           # step 0 is cold in both contexts
    summ = {"case": case, "summary": True, "steps": steps, "precond": precond,
            "cold_iterations": [r["cold"]["iterations"] for r in rows], "warm_iterations": [r["warm"]["iterations"] for r in rows],
            "cold_ms_mean_steps1plus": round(float(np.mean([r["cold"]["ms"] for r in later])), 2) if later else None,
            "warm_ms_mean_steps1plus": round(float(np.mean([r["warm"]["ms"] for r in later])), 2) if later else None,
            "iteration_ratio_steps1plus": round(sum(r["warm"]["iterations"] for r in later) / max(1, sum(r["cold"]["iterations"] for r in later)), 4) if later else None}
    emit(summ)
    return summ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="cavity128,cavity256,spheres256,coil256")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--precond", choices=list(PRECONDS), default="jacobi")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    f = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if f:
            f.write(line + "\n")
            f.flush()
    for case in args.cases.split(","):
        run_case(case, args.steps, PRECONDS[args.precond], emit)
    if f:
        f.close()


if __name__ == "__main__":
    main()

"""Free-slip solids (ps_set_solid_boundary) against no-slip, for profiles/solid_slip.md.
  python scripts/solid_slip.py [N] [STEPS]     coil and spheres at N^3 (default 256), Jacobi and Chebyshev-F32, bench.py's tolerance
                                               (1e-3): one context, the two modes alternating step by step after a warm-up step of
                                               each; per mode the median ms/step (Solver.step, host to host), setup ms, solve ms,
                                               iterations and solve ms per iteration, and the edges whose coupling free slip dropped"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(n, steps):
    import numpy as np
    import polystokes_amd
    from polystokes_amd import _abi as abi
    from polystokes_amd import scenes
    modes = (("no_slip", abi.SOLID_NO_SLIP), ("free_slip", abi.SOLID_FREE_SLIP))
    for scene in ("coil", "spheres"):
        sc, p = getattr(scenes, scene)(n)
        for pname, pre in (("jacobi", abi.PRE_DIAGONAL), ("chebyshev_f32", abi.PRE_CHEBYSHEV_F32)):
            p.preconditioner = pre
            s = polystokes_amd.Solver(0)
            rec = {m: {"ms": [], "setup": [], "solve": [], "it": []} for m, _ in modes}
            slip = 0
            for k in range(steps + 1):
                for m, mode in modes:
                    s.set_solid_boundary(mode)
                    t0 = time.perf_counter()
                    rc = s.step(sc, p)
                    ms = 1e3 * (time.perf_counter() - t0)
                    assert rc == abi.SUCCESS, (scene, pname, m, rc, s.last_error())
                    if mode == abi.SOLID_FREE_SLIP:
                        slip = int(s.array("solidSlipEdges")[0])
                    if k == 0:
                        continue                                      # warm-up
                    r = rec[m]
                    r["ms"].append(ms); r["setup"].append(s.stats.solveData[5]); r["solve"].append(s.stats.solveData[3])
                    r["it"].append(int(s.stats.solveData[1]))
            s.close()
            for m, _ in modes:
                r = rec[m]
                it = int(np.median(r["it"]))
                solve = float(np.median(r["solve"]))
                print(json.dumps({"scene": f"{scene}{n}", "precond": pname, "mode": m, "ms_per_step": round(float(np.median(r["ms"])), 2),
                                  "setup_ms": round(float(np.median(r["setup"])), 2), "solve_ms": round(solve, 2), "iterations": it,
                                  "solve_ms_per_iter": round(solve / max(it, 1), 4), "iterations_all": r["it"],
                                  "slip_edges": slip if m == "free_slip" else 0}), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 256, int(sys.argv[2]) if len(sys.argv) > 2 else 5)

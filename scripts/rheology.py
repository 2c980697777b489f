"""Non-Newtonian viscosity (ps_set_rheology): cost against the Newtonian path, for profiles/rheology.md.
  python scripts/rheology.py table [N] [STEPS]   coil and cavity at N^3 (default 256), bench.py's tolerance (1e-3), default parameters:
                                                 one context per mode, the modes alternating step by step after a warm-up step of each;
                                                 per mode the median setup ms, solve ms, iterations and solve ms per iteration.  Modes:
                                                 newtonian (the scene's constant viscosity), field (the mu of the law uploaded as a
                                                 Newtonian viscosity field), hb (Herschel-Bulkley n = 0.7, tau_y = 0, no pass)
  python scripts/rheology.py passes [N]          coil at N^3: the PCG iterations of each solve (array rheologyIterations) for passes
                                                 0, 1, 3, and the step's setup / solve ms
  python scripts/rheology.py step SCENE N MODEL  one warm-up step and one step of SCENE (coil | cavity) at N^3, MODEL newtonian | hb (for
                                                 a kernel trace: rocprofv3 --kernel-trace --stats -- python scripts/rheology.py step ...)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAW = dict(flow_index=0.7, yield_stress=0.0, min_shear_rate=1e-2, min_viscosity=1e-3, max_viscosity=1e6)


def _scene(name, n):
    from polystokes_amd import scenes
    return getattr(scenes, name)(n)


def table(n, steps):
    import numpy as np
    import polystokes_amd
    from polystokes_amd import _abi as abi
    for name in ("coil", "cavity"):
        sc, p = _scene(name, n)
        hb = polystokes_amd.Solver(0)
        hb.set_rheology(**LAW)
        assert hb.step(sc, p) == abi.SUCCESS, hb.last_error()
        mu = hb.array("rheologyViscosity").reshape(sc.viscosity.shape)
        sc_mu = abi.Scene(sc.nx, sc.ny, sc.nz, sc.dx, sc.dt, sc.density, sc.vel, sc.surface, sc.collision, mu, collisionvel=sc.collisionvel)
        runs = {"newtonian": (polystokes_amd.Solver(0), sc), "field": (polystokes_amd.Solver(0), sc_mu), "hb": (hb, sc)}
        rec = {m: {"setup": [], "solve": [], "it": []} for m in runs}
        for k in range(steps + 1):
            for m, (s, scene) in runs.items():
                rc = s.step(scene, p)
                assert rc == abi.SUCCESS, (name, m, rc, s.last_error())
                if k == 0:
                    continue                                          # warm-up
                rec[m]["setup"].append(s.stats.solveData[5]); rec[m]["solve"].append(s.stats.solveData[3])
                rec[m]["it"].append(int(s.stats.solveData[1]))
        for m, (s, _) in runs.items():
            r = rec[m]
            it = int(np.median(r["it"]))
            solve = float(np.median(r["solve"]))
            print(json.dumps({"scene": f"{name}{n}", "mode": m, "setup_ms": round(float(np.median(r["setup"])), 2), "solve_ms": round(solve, 2),
                              "iterations": it, "solve_ms_per_iter": round(solve / max(it, 1), 4), "iterations_all": r["it"]}), flush=True)
            s.close()


def passes(n):
    import polystokes_amd
    from polystokes_amd import _abi as abi
    sc, p = _scene("coil", n)
    for k in (0, 1, 3):
        s = polystokes_amd.Solver(0)
        s.set_rheology(passes=k, **LAW)
        assert s.step(sc, p) == abi.SUCCESS, s.last_error()                     # warm-up
        assert s.step(sc, p) == abi.SUCCESS, s.last_error()
        print(json.dumps({"scene": f"coil{n}", "passes": k, "iterations": [int(i) for i in s.array("rheologyIterations")],
                          "setup_ms": round(s.stats.solveData[5], 2), "solve_ms": round(s.stats.solveData[3], 2)}), flush=True)
        s.close()


def step(name, n, model):
    import polystokes_amd
    from polystokes_amd import _abi as abi
    sc, p = _scene(name, n)
    s = polystokes_amd.Solver(0)
    if model == "hb":
        s.set_rheology(**LAW)
    for _ in range(2):
        assert s.step(sc, p) == abi.SUCCESS, s.last_error()
    print(json.dumps({"scene": f"{name}{n}", "model": model, "iterations": int(s.stats.solveData[1]),
                      "setup_ms": round(s.stats.solveData[5], 2)}), flush=True)
    s.close()


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "table"
    if what == "table":
        table(int(sys.argv[2]) if len(sys.argv) > 2 else 256, int(sys.argv[3]) if len(sys.argv) > 3 else 5)
    elif what == "passes":
        passes(int(sys.argv[2]) if len(sys.argv) > 2 else 256)
    else:
        step(sys.argv[2], int(sys.argv[3]), sys.argv[4])

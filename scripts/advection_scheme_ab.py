#!/usr/bin/env python3
"""What ps_advect_fields_scheme_device costs with the MacCormack correction (profiles/advection_scheme.md), in the manner of advection_ab.py:
`spheres` at --res^3 after one step, order 2 with the context's carrier, three cell fields (the liquid SDF, the viscosity, a seeded random
field) and the velocity, torch tensors on the device in --layout, all on one caller's stream in one process, the candidates alternating:
  scheme       ps_advect_fields_scheme_device, scheme 1 with --limiter: the forward launch into the library's scratch and the correction launch
  plain        ps_advect_fields_device: the semi-Lagrangian call of the same library
  composed     what a caller builds today from outside: ps_advect_fields_device over dt (fields and velocity), ps_advect_fields_device over -dt
               on the three results, and out = hat + 0.5 * (f - bar) in torch.  No limiter (it needs the kernel's taps), and the velocity
               stays semi-Lagrangian: the call advects no face field but the carrier itself, so the reverse pass of the velocity cannot be composed
  scheme_cells / composed_cells    the same two for the three cell fields alone, where both compute the same correction (limiter none for the
               comparison of bytes: then the two agree to the last bit but for the fallback samples, which the composition does not know)
  copy         hipMemcpyAsync device-to-device of half the bytes a call must move: the carrier read once, the cell fields in and out, the velocity out
Each is --calls calls back to back, then one synchronisation of the stream: wall time / calls.  --rounds rounds after one warm-up round; the
table holds the median, the minimum and the maximum per call.  dt is chosen so that max|u| dt / dx = 3.7, as in advection_ab.py.
At --res up to 64 the outputs and the counters of `scheme` are compared with the numpy restatement, tests/advection_scheme_ref.py, byte for byte.
usage: advection_scheme_ab.py [--res 256] [--calls 50] [--rounds 5] [--order 2] [--limiter 1] [--layout 0] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--order", type=int, default=2)
    ap.add_argument("--limiter", type=int, default=1)
    ap.add_argument("--layout", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()                                                              # torch's HIP runtime first: it finds no device once the library has initialised its own
    import polystokes_amd
    from polystokes_amd import _abi as abi
    from polystokes_amd import scenes, from_layout, to_layout
    n = args.res
    sc, p = scenes.spheres(n, tile=16 if n >= 64 else 8)
    p.preconditioner = abi.PRE_DIAGONAL
    s = polystokes_amd.Solver(0)
    s.upload(sc, p)
    rc = s.step_device()
    vel, _ = s.download()
    top = max(float(np.abs(v).max()) for v in vel)
    dt = 3.7 * float(sc.dx) / top
    rng = np.random.RandomState(7)
    cells = [np.ascontiguousarray(sc.surface, np.float32), np.ascontiguousarray(sc.viscosity, np.float32).reshape(sc.surface.shape),
             rng.standard_normal(sc.surface.shape).astype(np.float32)]
    dev = torch.device("cuda", 0)
    cin = [torch.from_numpy(np.ascontiguousarray(to_layout(f, args.layout))).to(dev) for f in cells]
    cout, hat, bar = ([torch.empty_like(f) for f in cin] for _ in range(3))
    vout = [torch.empty(v.size, dtype=torch.float32, device=dev) for v in vel]
    st = torch.cuda.Stream(device=dev)
    MAC = abi.ADVECT_MACCORMACK

    def ok(rc):
        assert rc == abi.SUCCESS, s.last_error()

    def scheme(limiter=args.limiter, velocity=True):
        ok(s.advect_device(dt, cin, cout, order=args.order, carrier=None, vel_out=vout if velocity else None, layout=args.layout, stream=st, scheme=MAC, limiter=limiter))

    def plain():
        ok(s.advect_device(dt, cin, cout, order=args.order, carrier=None, vel_out=vout, layout=args.layout, stream=st))

    def composed(velocity=True):
        ok(s.advect_device(dt, cin, hat, order=args.order, carrier=None, vel_out=vout if velocity else None, layout=args.layout, stream=st))
        ok(s.advect_device(-dt, hat, bar, order=args.order, carrier=None, vel_out=None, layout=args.layout, stream=st))
        with torch.cuda.stream(st):
            for f, h, b, o in zip(cin, hat, bar, cout):
                torch.add(h, torch.sub(f, b, out=b), alpha=0.5, out=o)              # (in fp32: a caller's elementwise pass; bar is overwritten)

    def copy():
        with torch.cuda.stream(st):
            dst.copy_(src, non_blocking=True)

    def batch(fn):
        st.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        st.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.calls

    scheme()
    st.synchronize()
    counters, correction = s.array("advectionCounts").tolist(), s.array("advectionCorrection").tolist()
    checked = False
    if n <= 64:                                                                     # the restatement, where it is quick
        import advection_scheme_ref as sref
        want = sref.advect((sc.nx, sc.ny, sc.nz), float(sc.dx), dt, args.order, vel, cells, True, args.limiter)
        got = [from_layout(b.cpu().numpy(), f.shape, args.layout) for b, f in zip(cout + vout, cells + list(vel))]
        for a, b in zip(got, want[0] + want[1]):
            assert a.tobytes() == b.tobytes()
        assert counters == want[2].tolist() and correction == want[4].tolist() and float(s.array("advectionStep")[0]) == want[3], (counters, correction)
        checked = True
    # the composition next to the fused call on the cell fields, limiter none: where no sample falls back the two differ only by the fp32 combine
    scheme(abi.ADVECT_LIMIT_NONE, False)
    st.synchronize()
    fused = [o.clone() for o in cout]
    composed(False)
    st.synchronize()
    agree = [float((a == b).float().mean()) for a, b in zip(fused, cout)]
    nc, nf = cells[0].size, sum(v.size for v in vel)
    nbytes = 4 * (nf + 2 * len(cells) * nc + nf)
    nbytes -= nbytes % 16
    src, dst = (torch.empty(nbytes // 8, dtype=torch.float32, device=dev) for _ in range(2))      # nbytes / 2 bytes each
    dst.copy_(src)
    runs = {"copy": copy, "scheme": scheme, "plain": plain, "composed": composed, "scheme_cells": lambda: scheme(velocity=False),
            "composed_cells": lambda: composed(False)}
    times = {k: [] for k in runs}
    for r in range(args.rounds + 1):
        for k, fn in runs.items():
            t = batch(fn)
            if r:                                                                  # (the first round warms up)
                times[k].append(t)
    med = {k: float(np.median(v)) for k, v in times.items()}
    out = {"res": n, "order": args.order, "limiter": args.limiter, "layout": args.layout, "cell_fields": len(cells), "calls": args.calls, "rounds": args.rounds,
           "cells": nc, "faces": nf, "bytes": nbytes, "dt": dt, "r": float(s.array("advectionStep")[0]), "step_rc": int(rc),
           "ms": times, "ms_median": med, "scheme_over_composed": med["scheme"] / med["composed"], "scheme_over_copy": med["scheme"] / med["copy"],
           "scheme_over_plain": med["scheme"] / med["plain"], "scheme_cells_over_composed_cells": med["scheme_cells"] / med["composed_cells"],
           "counters": counters, "correction": correction, "compared_with_restatement": checked, "cells_equal_to_composition_share": agree,
           "scratch_bytes": 4 * (len(cells) * nc + nf), "library": polystokes_amd.LIB_PATH}
    s.close()
    print("RESULT " + json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

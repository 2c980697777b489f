#!/usr/bin/env python3
"""What ps_advect_fields_device costs (profiles/advection.md): `spheres` at --res^3 after one step, order 2 with the context's carrier (the
velocity that step wrote), three cell fields (the liquid SDF, the viscosity, a seeded random field) and the velocity itself, device arrays,
x fastest, next to a device-to-device copy that moves the same number of bytes, on the same device in the same process, alternating.
  advect  --calls device-form calls back to back on a caller's stream (no host synchronisation between them), then one synchronisation of
          that stream, which waits for the last result: wall time / calls.  A call is the counters' reset, the kernel and the two event
          hand-overs between the caller's stream and the context's.
  copy    --calls hipMemcpyAsync device-to-device of half the bytes the call must move (the copy reads and writes each of them), then a
          stream synchronisation: wall time / calls
The bytes a call must move: the three carrier grids read once, the cell fields in and out, the velocity out.  dt is chosen so that
max|u| dt / dx = 3.7.  --rounds rounds after one warm-up round; the table holds the median, the minimum and the maximum per call.
At --res 32 (any res up to 64) the outputs and the counters are compared with the numpy restatement, tests/advection_ref.py, byte for byte.
usage: advection_ab.py [--res 256] [--calls 50] [--rounds 5] [--order 2] [--layout 0] [--out FILE.json]"""
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
    ap.add_argument("--layout", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import polystokes_amd
    from polystokes_amd import _abi as abi
    from polystokes_amd import _hip, scenes, from_layout, to_layout
    n = args.res
    sc, p = scenes.spheres(n, tile=16 if n >= 64 else 8)
    p.preconditioner = abi.PRE_DIAGONAL
    s = polystokes_amd.Solver(0)
    s.upload(sc, p)
    t0 = time.perf_counter()
    rc = s.step_device()
    step_ms = (time.perf_counter() - t0) * 1e3
    vel, _ = s.download()
    top = max(float(np.abs(v).max()) for v in vel)
    dt = 3.7 * float(sc.dx) / top
    rng = np.random.RandomState(7)
    cells = [np.ascontiguousarray(sc.surface, np.float32), np.ascontiguousarray(sc.viscosity, np.float32).reshape(sc.surface.shape),
             rng.standard_normal(sc.surface.shape).astype(np.float32)]
    cin = [_hip.DeviceBuffer.from_numpy(to_layout(f, args.layout)) for f in cells]
    cout = [_hip.DeviceBuffer(f.size) for f in cells]
    vout = [_hip.DeviceBuffer(v.size) for v in vel]
    st = _hip.Stream()

    def advect_batch():
        t0 = time.perf_counter()
        for _ in range(args.calls):
            assert s.advect_device(dt, cin, cout, order=args.order, carrier=None, vel_out=vout, layout=args.layout, stream=st) == abi.SUCCESS, s.last_error()
        st.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.calls

    advect_batch()
    counters = s.array("advectionCounts").tolist()
    checked = False
    if n <= 64:                                                                     # the restatement, where it is quick
        import advection_ref as ref
        want = ref.advect((sc.nx, sc.ny, sc.nz), float(sc.dx), dt, args.order, vel, cells, True)
        got = [from_layout(b.to_numpy(), f.shape, args.layout) for b, f in zip(cout + vout, cells + list(vel))]
        for a, b in zip(got, want[0] + want[1]):
            assert a.tobytes() == b.tobytes()
        assert counters == want[2].tolist() and float(s.array("advectionStep")[0]) == want[3], (counters, want[2].tolist())
        checked = True
    nc, nf = cells[0].size, sum(v.size for v in vel)
    nbytes = 4 * (nf + 2 * len(cells) * nc + nf)
    nbytes -= nbytes % 16
    src, dst = _hip.DeviceBuffer(nbytes // 8), _hip.DeviceBuffer(nbytes // 8)      # nbytes / 2 bytes each
    _hip.memcpy(src.ptr, dst.ptr, src.nbytes, _hip.D2D)                             # (touch both)

    def copy_batch():
        t0 = time.perf_counter()
        for _ in range(args.calls):
            _hip.memcpy_async(dst.ptr, src.ptr, src.nbytes, _hip.D2D, st.cuda_stream)
        st.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.calls

    advect, copy = [], []
    for r in range(args.rounds + 1):
        c = copy_batch()
        q = advect_batch()
        if r:                                                                      # (the first round warms up)
            copy.append(c)
            advect.append(q)
    out = {"res": n, "order": args.order, "layout": args.layout, "cell_fields": len(cells), "calls": args.calls, "rounds": args.rounds,
           "cells": nc, "faces": nf, "bytes": nbytes, "dt": dt, "r": float(s.array("advectionStep")[0]), "step_rc": int(rc), "step_ms": step_ms,
           "advect_ms": advect, "copy_ms": copy, "advect_ms_median": float(np.median(advect)), "copy_ms_median": float(np.median(copy)),
           "ratio": float(np.median(advect) / np.median(copy)), "advect_GBps": nbytes / np.median(advect) / 1e6,
           "copy_GBps": nbytes / np.median(copy) / 1e6, "counters": counters, "compared_with_restatement": checked,
           "library": polystokes_amd.LIB_PATH}
    st.close()
    for b in cin + cout + vout + [src, dst]:
        b.close()
    s.close()
    print("RESULT " + json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

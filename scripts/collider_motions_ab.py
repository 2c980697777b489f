#!/usr/bin/env python3
"""What ps_paint_collider_velocities costs (profiles/collider_motions.md): `spheres` at --res^3 with 8 colliders and the nearest-sphere id
field, next to a device-to-device copy that moves the same number of bytes, on the same device in the same process, alternating.
  paint   --calls device-form calls back to back (no host synchronisation between them), then one read of the counters, which ends with the
          context's stream synchronised: wall time / calls.  A call is the table's copy, the counters' reset and the kernel.
  copy    --calls hipMemcpyAsync device-to-device of half the bytes the kernel must move (the copy reads and writes each of them), then a
          stream synchronisation: wall time / calls
The bytes the kernel must move: the three face grids written, `collision` and the ids read once (the neighbouring cell's second read is
taken to come from cache).  --rounds rounds after one warm-up round; the table holds the median, the minimum and the maximum per call.
usage: collider_motions_ab.py [--res 256] [--calls 50] [--rounds 5] [--out FILE.json]"""
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import polystokes_amd
    from polystokes_amd import _abi as abi
    from polystokes_amd import _hip, scenes
    import collider_motions_cases as cases
    n = args.res
    sc, p = scenes.spheres(n, tile=16)
    ids = cases.ids_field(sc, "spheres")
    tab = cases.table("spheres", 8)
    faces = 3 * n * n * (n + 1)
    nbytes = 4 * faces + 2 * 4 * n ** 3
    s = polystokes_amd.Solver(0)
    s.upload(sc, p)
    assert s.upload_collider_ids(ids) == abi.SUCCESS, s.last_error()
    dev_tab = _hip.DeviceBuffer.from_numpy(tab.view(np.float32))
    src, dst = _hip.DeviceBuffer(nbytes // 8), _hip.DeviceBuffer(nbytes // 8)      # nbytes / 2 bytes each
    _hip.memcpy(src.ptr, dst.ptr, src.nbytes, _hip.D2D)                             # (touch both)
    st = _hip.Stream()

    def paint_batch():
        t0 = time.perf_counter()
        for _ in range(args.calls):
            assert s.paint_collider_velocities_device(dev_tab, 8, st) == abi.SUCCESS, s.last_error()
        counters = s.array("colliderMotionFaces")                                  # ends with the context's stream synchronised
        return (time.perf_counter() - t0) * 1e3 / args.calls, counters

    def copy_batch():
        t0 = time.perf_counter()
        for _ in range(args.calls):
            _hip.memcpy_async(dst.ptr, src.ptr, src.nbytes, _hip.D2D, st.cuda_stream)
        st.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.calls

    paint, copy = [], []
    for r in range(args.rounds + 1):
        c = copy_batch()
        q, counters = paint_batch()
        if r:                                                                      # (the first round warms up)
            copy.append(c)
            paint.append(q)
    t0 = time.perf_counter()
    assert s.paint_collider_velocities(tab) == abi.SUCCESS                         # the host form: it ends synchronised
    host_ms = (time.perf_counter() - t0) * 1e3
    want = None
    if n <= 64:                                                                    # the restatement, where it is quick
        import collider_motions_ref as ref
        want = ref.paint(sc.collision, ids, tab, (0.0, 0.0, 0.0), sc.dx, 1, sc.collisionvel)[1].tolist()
        assert counters.tolist() == want, (counters.tolist(), want)
    out = {"res": n, "colliders": 8, "calls": args.calls, "rounds": args.rounds, "faces": faces, "bytes": nbytes,
           "paint_ms": paint, "copy_ms": copy, "paint_ms_median": float(np.median(paint)), "copy_ms_median": float(np.median(copy)),
           "ratio": float(np.median(paint) / np.median(copy)), "paint_GBps": nbytes / np.median(paint) / 1e6,
           "copy_GBps": nbytes / np.median(copy) / 1e6, "host_form_ms": host_ms, "counters": counters.tolist(),
           "library": polystokes_amd.LIB_PATH}
    st.close()
    for b in (dev_tab, src, dst):
        b.close()
    s.close()
    print("RESULT " + json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What ps_place_colliders costs (profiles/collider_shapes.md): the 8 spheres of `spheres` at --res^3 as eight 48^3 volumes under random
rotations, placed into a collision field without solids, next to a device-to-device copy that moves the same number of bytes, on the same
device in the same process, alternating.
  place   --calls device-form calls back to back (no host synchronisation between them), then one read of the counters, which ends with the
          context's stream synchronised: wall time / calls.  A call is the poses' copy, the counters' reset and the kernel.
  copy    --calls hipMemcpyAsync device-to-device of half the bytes the kernel must move (the copy reads and writes each of them), then a
          stream synchronisation: wall time / calls
The bytes a call must move: `collision` read, `collision` and the ids written where a collider wins, the volumes once.  Only the first
call after an upload wins cells: the calls after it find their own values, evaluate every collider again and write nothing, so the
steady-state bytes hold no writes; the first call is timed on its own (a host-form call, which ends synchronised).
--rounds rounds after one warm-up round; the table holds the median, the minimum and the maximum per call.
usage: collider_shapes_ab.py [--res 256] [--calls 50] [--rounds 5] [--out FILE.json]"""
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
    import collider_loads_cases as loads_cases
    import collider_shapes_cases as cases
    n = args.res
    sc, p = scenes.spheres(n, tile=16)
    sc.collision[...] = 10.0                                                        # no solids: the placement brings the spheres
    rng = np.random.RandomState(3)
    shapes, poses = [], []
    for c, rad in loads_cases.sphere_table():
        shape = cases.sphere_volume(rad, 48, 2.4 * rad / 48.0)
        shapes.append(shape)
        poses.append(cases.pose(shape, cases.rotation(rng), c))
    poses = np.array(poses)
    samples = 8 * 48 ** 3
    s = polystokes_amd.Solver(0)
    assert s.set_collider_shapes(shapes) == abi.SUCCESS, s.last_error()
    s.upload(sc, p)
    t0 = time.perf_counter()
    assert s.place_colliders(poses) == abi.SUCCESS, s.last_error()                   # the first call: it wins the spheres' cells
    first_ms = (time.perf_counter() - t0) * 1e3
    first = s.array("colliderPlacedCells").tolist()
    want = None
    if n <= 64:                                                                     # the restatement, where it is quick
        import collider_shapes_ref as ref
        want = ref.place(np.full_like(sc.collision, 10.0), None, shapes, poses, (0.0, 0.0, 0.0), sc.dx, 1)[2].tolist()
        assert first == want, (first, want)
    dev = _hip.DeviceBuffer.from_numpy(poses.view(np.float32))
    st = _hip.Stream()

    def place_batch():
        t0 = time.perf_counter()
        for _ in range(args.calls):
            assert s.place_colliders_device(dev, 8, st) == abi.SUCCESS, s.last_error()
        counters = s.array("colliderPlacedCells")                                  # ends with the context's stream synchronised
        return (time.perf_counter() - t0) * 1e3 / args.calls, counters

    _, counters = place_batch()
    nbytes = 4 * n ** 3 + 8 * int(counters[:8].sum()) + 4 * samples
    nbytes -= nbytes % 16
    src, dst = _hip.DeviceBuffer(nbytes // 8), _hip.DeviceBuffer(nbytes // 8)      # nbytes / 2 bytes each
    _hip.memcpy(src.ptr, dst.ptr, src.nbytes, _hip.D2D)                             # (touch both)

    def copy_batch():
        t0 = time.perf_counter()
        for _ in range(args.calls):
            _hip.memcpy_async(dst.ptr, src.ptr, src.nbytes, _hip.D2D, st.cuda_stream)
        st.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.calls

    place, copy = [], []
    for r in range(args.rounds + 1):
        c = copy_batch()
        q, counters = place_batch()
        if r:                                                                      # (the first round warms up)
            copy.append(c)
            place.append(q)
    out = {"res": n, "colliders": 8, "calls": args.calls, "rounds": args.rounds, "cells": n ** 3, "volume_samples": samples, "bytes": nbytes,
           "first_call_bytes": 4 * n ** 3 + 8 * int(np.sum(first[:8])) + 4 * samples, "first_call_host_form_ms": first_ms,
           "place_ms": place, "copy_ms": copy, "place_ms_median": float(np.median(place)), "copy_ms_median": float(np.median(copy)),
           "ratio": float(np.median(place) / np.median(copy)), "place_GBps": nbytes / np.median(place) / 1e6,
           "copy_GBps": nbytes / np.median(copy) / 1e6, "first_counters": first, "counters": counters.tolist(),
           "library": polystokes_amd.LIB_PATH}
    st.close()
    for b in (dev, src, dst):
        b.close()
    s.close()
    print("RESULT " + json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

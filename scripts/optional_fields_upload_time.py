#!/usr/bin/env python3
"""Host wall time of ps_upload_fields on the 128^3 coil with no optional cell field present and with all four (density, sigma + ambient
pressure, contact cosine, collider ids) uploaded before each call, so that the upload has them to drop.  PS_LIB selects the library.

    python scripts/optional_fields_upload_time.py [--res 128] [--calls 20]

One JSON line: median, min and max in ms of `calls` uploads per case (two more are run first and discarded)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import polystokes_amd  # noqa: E402
from polystokes_amd import _abi as abi  # noqa: E402
from polystokes_amd import scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    sc, p = scenes.coil(a.res)
    sh = sc.surface.shape
    rng = np.random.RandomState(1)
    rho = (900.0 * (1.0 + rng.uniform(0, 1, sh))).astype(np.float32)
    sig, pres = rng.uniform(0.1, 1, sh).astype(np.float32), rng.uniform(-5, 5, sh).astype(np.float32)
    cos, ids = rng.uniform(-1, 1, sh).astype(np.float32), rng.randint(0, 2, sh).astype(np.int32)
    s = polystokes_amd.Solver(0)
    fi = sc.fields_in()
    s.scene = sc
    out = {"lib": polystokes_amd.LIB_PATH, "res": a.res, "calls": a.calls}
    for case in ("none_present", "all_four_present"):
        ms = []
        for _ in range(a.calls + 2):
            if case == "all_four_present":
                assert s.upload_density_field(rho) == abi.SUCCESS and s.upload_surface_fields(sig, pres) == abi.SUCCESS
                assert s.upload_contact_cosine_field(cos) == abi.SUCCESS and s.upload_collider_ids(ids) == abi.SUCCESS
            t0 = time.perf_counter()
            rc = s.L.ps_upload_fields(s.h, C.byref(p), C.byref(fi))
            ms.append(1e3 * (time.perf_counter() - t0))
            assert rc == abi.SUCCESS
        ms = sorted(ms[2:])
        out[case] = {"median_ms": round(ms[len(ms) // 2], 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3)}
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

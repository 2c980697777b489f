#!/usr/bin/env python3
"""What ps_label_air_pockets costs (profiles/air_pockets.md): the wall time around the call (it ends with the stream synchronised), the
median of --calls calls after 2 warm-ups on one context, next to the setup time of the same upload (the sum of stage_ms[0..7], three
setups), on two scenes at --res^3: `coil`, and the pool with two bubbles of tests/air_pockets_cases.py scaled up.
One child process per (library, scene):
  this     this tree's library
  plain    this tree's objects with ps_pockets.hip rebuilt under -DPS_POCKETS_PLAIN_ATOMICS (--build-plain builds it first, into
           polystokes_amd/variants/lib_pockets_plain.so): every lane its own atomics in k_pocket_sums
  parent   the library of another checkout (--parent DIR: that tree's polystokes_amd/ with its built library), which has no such call:
           its setup time alone
usage: air_pockets_ab.py [--build-plain] [--parent DIR] [--res 256] [--calls 10] [--out FILE.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polystokes_amd", "csrc")
PLAIN = os.path.join(ROOT, "polystokes_amd", "variants", "lib_pockets_plain.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off"]


def build_plain():
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j8", "../libpolystokes_hip.so"])
    build = os.path.join(CSRC, "_build")
    os.makedirs(os.path.join(build, "pockets_plain"), exist_ok=True)
    os.makedirs(os.path.dirname(PLAIN), exist_ok=True)
    obj = os.path.join(build, "pockets_plain", "ps_pockets.o")
    subprocess.check_call([HIPCC] + FLAGS + ["-DPS_POCKETS_PLAIN_ATOMICS", "-c", os.path.join(CSRC, "ps_pockets.hip"), "-o", obj])
    others = sorted(os.path.join(build, f) for f in os.listdir(build) if f.endswith(".o") and f != "ps_pockets.o")
    subprocess.check_call([HIPCC, "-shared", "-fPIC", "--offload-arch=gfx950", "-o", PLAIN] + others + [obj])


def child(scene, res, calls, label, package_root):
    sys.path.insert(0, package_root)
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import numpy as np
    import polystokes_amd
    from polystokes_amd import scenes
    import air_pockets_cases as cases
    sc, p = scenes.coil(res) if scene == "coil" else cases.bubbles_scaled(res)
    s = polystokes_amd.Solver(0)
    s.upload(sc, p)
    out = {"scene": scene, "res": res, "library": polystokes_amd.LIB_PATH}
    if label:
        times = []
        for _ in range(calls + 2):
            t0 = time.perf_counter()
            k = s.label_air_pockets()
            times.append((time.perf_counter() - t0) * 1e3)
        out.update(K=k, passes=int(s.array("airPocketPasses")[0]), label_ms_median=float(np.median(times[2:])), label_ms_min=min(times[2:]),
                   label_ms_max=max(times[2:]), label_ms_warmups=times[:2], cells=[int(v) for v in s.array("airPocketCells")[:8]],
                   units=[int(v) for v in s.array("airPocketUnits")[:8]], open=[int(v) for v in s.array("airPocketOpen")[:8]])
    setups = []
    for _ in range(3):
        s.setup()
        setups.append(sum(s.stats.stage_ms[i] for i in range(8)))
    out["setup_ms"] = setups
    s.close()
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-plain", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=3, metavar=("SCENE", "LABEL", "PACKAGE_ROOT"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child[0], args.res, args.calls, args.child[1] == "1", args.child[2])
        sys.exit(0)
    if args.build_plain:
        build_plain()
    runs = [("this", None, True, ROOT)]
    if os.path.exists(PLAIN):
        runs.append(("plain", PLAIN, True, ROOT))
    if args.parent:
        runs.append(("parent", None, False, os.path.abspath(args.parent)))
    results = {}
    for scene in ("coil", "bubbles"):
        for tag, lib, label, package_root in runs:
            env = dict(os.environ)
            env.pop("PS_LIB", None)
            if lib:
                env["PS_LIB"] = lib
            pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--res", str(args.res), "--calls", str(args.calls), "--child", scene,
                                 "1" if label else "0", package_root], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if pr.returncode != 0:
                sys.exit("%s %s failed (%d):\n%s" % (tag, scene, pr.returncode, pr.stdout[-3000:]))      # nothing more is started on the GPU
            line = [l for l in pr.stdout.splitlines() if l.startswith("RESULT ")][-1]
            results["%s_%s" % (tag, scene)] = json.loads(line[7:])
    if "plain_coil" in results:      # the A/B changes the time and nothing else
        for scene in ("coil", "bubbles"):
            for key in ("K", "cells", "units", "open"):
                assert results["this_" + scene][key] == results["plain_" + scene][key], (scene, key)
    print(json.dumps(results, indent=1), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)

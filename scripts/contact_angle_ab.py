#!/usr/bin/env python3
"""What the contact-angle rule (ps_set_contact_angle) adds to a setup (profiles/contact_angle.md): two contexts of this tree's library in
one process take the same upload of a --res^3 scene with sigma > 0, one with the angle off and one with --angle degrees, and run
ps_setup_device in turns (off, on, off, on, ...), --setups each after 2 warm-ups each (the first setups pay the allocations).  Per setup:
stage_ms[PS_STAGE_ASSEMBLE] (device events around the stage that holds the curvature and, ahead of it, the rule) and the sum of
stage_ms[0..7].  Reported: median, min and max of each, and the differences of the medians.  One child process per scene (`coil`,
`spheres`); `--child SCENE` runs one alone, e.g. under a kernel trace.
usage: contact_angle_ab.py [--res 256] [--setups 10] [--angle 60] [--sigma 0.07] [--out FILE.json]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE_ASSEMBLE = 6


def child(scene, res, setups, angle, sigma):
    sys.path.insert(0, ROOT)
    import numpy as np
    import polystokes_amd
    from polystokes_amd import scenes
    sc, p = {"coil": scenes.coil, "spheres": scenes.spheres}[scene](res)
    sc.surface_tension = sigma
    ctx = {}
    for tag, deg in (("off", -1.0), ("on", angle)):
        s = polystokes_amd.Solver(0)
        assert s.set_contact_angle(deg) == 1
        s.upload(sc, p)
        ctx[tag] = s
    times = {tag: {"assemble": [], "setup": []} for tag in ctx}
    for it in range(setups + 2):
        for tag in ("off", "on"):
            s = ctx[tag]
            s.setup()
            if it >= 2:
                times[tag]["assemble"].append(float(s.stats.stage_ms[STAGE_ASSEMBLE]))
                times[tag]["setup"].append(float(sum(s.stats.stage_ms[i] for i in range(8))))
    on = ctx["on"]
    out = {"scene": scene, "res": res, "angle": angle, "sigma": sigma, "library": polystokes_amd.LIB_PATH,
           "contactCells": int(on.array("contactCells")[0]), "cells": sc.nx * sc.ny * sc.nz}
    try:
        ctx["off"].array("surfaceWetted")
        raise AssertionError("the context with the angle off ran the rule")
    except KeyError:
        pass
    out["curvature_changed_cells"] = int((on.array("surfaceCurvature") != ctx["off"].array("surfaceCurvature")).sum())
    for tag in ctx:
        for key, v in times[tag].items():
            out["%s_%s_ms" % (tag, key)] = {"median": float(np.median(v)), "min": min(v), "max": max(v), "all": v}
    for key in ("assemble", "setup"):
        out["added_%s_ms" % key] = out["on_%s_ms" % key]["median"] - out["off_%s_ms" % key]["median"]
    for s in ctx.values():
        s.close()
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--setups", type=int, default=10)
    ap.add_argument("--angle", type=float, default=60.0)
    ap.add_argument("--sigma", type=float, default=0.07)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, metavar="SCENE", help="run one scene in this process")
    args = ap.parse_args()
    if args.child:
        child(args.child, args.res, args.setups, args.angle, args.sigma)
        sys.exit(0)
    results = {}
    for scene in ("coil", "spheres"):
        env = dict(os.environ)
        env.pop("PS_LIB", None)
        pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--res", str(args.res), "--setups", str(args.setups), "--angle", str(args.angle),
                             "--sigma", str(args.sigma), "--child", scene], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if pr.returncode != 0:
            sys.exit("%s failed (%d):\n%s" % (scene, pr.returncode, pr.stdout[-3000:]))      # nothing more is started on the GPU
        line = [l for l in pr.stdout.splitlines() if l.startswith("RESULT ")][-1]
        results[scene] = json.loads(line[7:])
    print(json.dumps(results, indent=1), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)

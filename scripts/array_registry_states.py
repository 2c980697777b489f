#!/usr/bin/env python3
"""What ps_query_array answers for every array name of the library, state by state: a dump to compare between two builds (PS_LIB selects
the library; the two dumps must be byte-identical when a change is meant to leave the registry alone).

    python scripts/array_registry_states.py OUT.txt
    PS_LIB=<other build>/libpolystokes_hip.so python scripts/array_registry_states.py OTHER.txt && cmp OUT.txt OTHER.txt

States, on one context and a 24 x 20 x 28 blob with surface tension: fresh, upload, optional fields uploaded, setup, solve,
set_velocity_extrapolation(2) + step, set_velocity_extrapolation(0), collider loads on + step, off, contact angle on + step, off,
label pockets, setup with the labels, re-upload; then, in a child process whose allocations are capped (PS_DEBUG_ALLOC_LIMIT, lab build),
a setup that throws with every optional field and the labels present.  One line per state and name: count and element bytes (-1 0: absent).
NAMES is the one explicit list: every name of include/polystokes.h and of ps_context::registerArrays."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import polystokes_amd  # noqa: E402
from polystokes_amd import _abi as abi  # noqa: E402
from polystokes_amd import scenes  # noqa: E402

SAMPLES = ("center", "faceX", "faceY", "faceZ", "edgeYZ", "edgeXZ", "edgeXY")
NAMES = [s + k for s in SAMPLES for k in ("LiquidWeights", "FluidWeights", "Labels", "ActiveIndices", "ReducedIndices")] + [
    "reducedRegionCOM", "reducedRegionCenterOfMass", "reducedRegionBestFitVectors", "reducedMassMatrices", "reducedViscosityMatrices",
    "Inv_Mr_plus_2JDtuDJ", "reducedRHSVector", "McInv", "activeRHSVector", "oldActiveVs", "uInv", "Mc", "u", "pressureRHSVector",
    "stressRHSVector", "b", "solutionVector", "guessVector", "warmStartVector", "warmStartUsed", "solvePrecisionUsed",
    "solvePassIterations", "solveTrueResidual", "densityField", "surfaceTension", "surfaceFields", "surfaceCurvature",
    "surfaceTensionReducedFaces", "surfaceGhostPressure", "contactAngle", "contactCosine", "contactField", "contactCells", "surfaceWetted",
    "solidBoundary", "solidSlipEdges", "rheologyModel", "rheologyStrainRate", "rheologyViscosity", "rheologyIterations",
    "velocityExtrapolation", "extrapolationLayerX", "extrapolationLayerY", "extrapolationLayerZ", "extrapolationCounts",
    "colliderLoads", "colliderForce", "colliderTorque", "colliderLoadScale", "colliderLoadTerms", "dinv", "recoveredActiveVelocity",
    "recoveredReducedVelocity", "valuesCoded", "diagonalsCoded", "columns16", "fusedStep", "ownedRange", "launchWalk", "chebInner32",
    "streamRuns", "rowPerLane", "sysPerm", "rowPerm", "S.ptr", "S.col", "S.val", "St.ptr", "St.col", "St.val", "S.chunkInfo", "S.chunkRep",
    "St.chunkInfo", "St.chunkRep", "S.code", "St.code", "reducedRowFace", "reducedRowRegion",
    "velX", "velY", "velZ", "validX", "validY", "validZ", "faceRowX", "faceRowY", "faceRowZ", "ownedX", "ownedY", "ownedZ",
    "airPockets", "airPocketIds", "airPocketUnits", "airPocketCells", "airPocketOpen", "airPocketVolume", "airPocketPasses",
]


def dump(s, state, out):
    for name in NAMES:
        eb = C.c_int32(0)
        n = s.L.ps_query_array(s.h, name.encode(), C.byref(eb))
        out.append("%s %s %d %d" % (state, name, n, eb.value if n >= 0 else 0))


def scene_and_fields():
    sc, p = scenes.blob(seed=2)
    sc.surface_tension = 0.5
    rng = np.random.RandomState(5)
    sh = sc.surface.shape
    return sc, p, dict(density=(900.0 * (1.0 + rng.uniform(0, 1, sh))).astype(np.float32), sigma=rng.uniform(0.1, 1.0, sh).astype(np.float32),
                       pressure=rng.uniform(-5, 5, sh).astype(np.float32), cosine=rng.uniform(-1, 1, sh).astype(np.float32),
                       ids=rng.randint(0, 2, sh).astype(np.int32))


def upload_optional(s, f):
    assert s.upload_density_field(f["density"]) == abi.SUCCESS
    assert s.upload_surface_fields(f["sigma"], f["pressure"]) == abi.SUCCESS
    assert s.upload_contact_cosine_field(f["cosine"]) == abi.SUCCESS
    assert s.upload_collider_ids(f["ids"]) == abi.SUCCESS


def throwing_child():
    """stdout: the state after a setup that ran out of (capped) memory, every optional field and the pocket labels present"""
    sc, p, f = scene_and_fields()
    s = polystokes_amd.Solver(0)
    s.upload(sc, p)
    upload_optional(s, f)
    s.label_air_pockets()
    out = []
    try:
        s.setup()
        out.append("setup_that_throws DID_NOT_THROW 0 0")
    except polystokes_amd.PolyStokesError:
        pass
    dump(s, "setup_that_throws", out)
    s.close()
    print("\n".join(out))


def main():
    if sys.argv[1] == "--throwing-child":
        return throwing_child()
    sc, p, f = scene_and_fields()
    s = polystokes_amd.Solver(0)
    out = []
    dump(s, "fresh", out)
    s.upload(sc, p)
    dump(s, "upload", out)
    upload_optional(s, f)
    dump(s, "optional_fields", out)
    held = s.memory_stats()["live_bytes"]
    s.setup()
    dump(s, "setup", out)
    peak = s.memory_stats()["peak_bytes"]
    s.solve()
    dump(s, "solve", out)
    s.set_velocity_extrapolation(2)
    s.step_device()
    dump(s, "extrapolation_2_step", out)
    s.set_velocity_extrapolation(0)
    dump(s, "extrapolation_0", out)
    s.set_collider_loads(2)
    s.step_device()
    dump(s, "collider_loads_on_step", out)
    s.set_collider_loads(0)
    dump(s, "collider_loads_off", out)
    s.set_contact_angle(60.0)
    s.step_device()
    dump(s, "contact_angle_on_step", out)
    s.upload_contact_cosine_field(None)
    s.set_contact_angle(-1.0)
    dump(s, "contact_angle_off", out)
    s.label_air_pockets()
    dump(s, "label_pockets", out)
    s.setup()
    dump(s, "setup_with_labels", out)
    s.upload_surface_fields(None, None)
    dump(s, "surface_fields_dropped", out)
    s.upload(sc, p)
    dump(s, "re_upload", out)
    s.close()
    # a setup that throws: the cap lies between what the uploads hold and what the setup needs
    env = dict(os.environ, PS_DEBUG_ALLOC_LIMIT=str(held + (peak - held) // 2))
    pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--throwing-child"], stdout=subprocess.PIPE, text=True, env=env, timeout=300)
    assert pr.returncode == 0
    out += [l for l in pr.stdout.splitlines() if l.startswith("setup_that_throws ")]
    with open(sys.argv[1], "w") as fh:
        fh.write("\n".join(out) + "\n")
    print("%d lines, %d states" % (len(out), len(out) // len(NAMES)))


if __name__ == "__main__":
    main()

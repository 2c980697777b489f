#!/usr/bin/env python3
"""The per-tile setup (region boxes, face offsets from the tiles' centres, face-box and union-box work items) as eight small cases in ONE
process, each dumped to OUT/<case>.npz: the tile arrays, the skin-row numbering, S, b, the Jacobi diagonal, the solution, the velocities
and valid masks, result, error and iterations; for the two eight-rank cases one file per rank, for the export case the bytes of every file
written.  Run it on two checkouts (--root) with the same switches (none, PS_TILE_VALU=1, PS_TILE_CLASS_MASK=3: read once per process),
then `solve_stages_cases.py --compare A B` says whether every array is identical byte for byte (profiles/region_box.md).
usage: region_box_cases.py OUT [--root CHECKOUT]"""
import os, sys, tempfile

ARRAYS = ("reducedRegionCOM", "reducedRegionBestFitVectors", "reducedMassMatrices", "reducedViscosityMatrices", "Inv_Mr_plus_2JDtuDJ",
          "reducedRHSVector", "reducedRowFace", "reducedRowRegion", "faceRowX", "faceRowY", "faceRowZ", "S.ptr", "S.col", "S.code", "b", "dinv",
          "solutionVector")


def main(out, root):
    sys.path.insert(0, root)
    import numpy as np
    import polystokes_amd
    from polystokes_amd import scenes, _abi as abi
    os.makedirs(out, exist_ok=True)

    def arrays(s):
        d, missing = {}, []
        for a in ARRAYS:
            try:
                d[a] = np.asarray(s.array(a)).copy()
            except KeyError:
                d[a] = np.zeros(0); missing.append(a)
        return d, missing

    def jacobi(case):                              # (the Jacobi diagonal exists as "dinv" with this preconditioner only)
        sc, p = case
        p.preconditioner = abi.PRE_DIAGONAL
        return sc, p

    def single(name, sc, p, export=False):
        s = polystokes_amd.Solver(0)
        rc = s.step(sc, p)
        d, missing = arrays(s)
        d.update(rc=np.int32(rc), solveData=np.array(s.stats.solveData[:], np.float64))
        for a in range(3):
            d["vel" + "XYZ"[a]], d["valid" + "XYZ"[a]] = s.vel[a], s.valid[a]
        if export:
            with tempfile.TemporaryDirectory() as tmp:
                s.export_matrices(os.path.join(tmp, "m_"))
                s.export_component_matrices(os.path.join(tmp, "c_"))
                for f in sorted(os.listdir(tmp)):
                    d["file:" + f] = np.frombuffer(open(os.path.join(tmp, f), "rb").read(), np.uint8)
        np.savez(os.path.join(out, name + ".npz"), **d)
        print("%-22s rc %d iterations %d regions %d arrays %d missing %s" % (name, rc, int(d["solveData"][1]), s.nRegions, len(d), missing), flush=True)
        s.close()

    def bricks(name, sc, p):
        grp = polystokes_amd.Group(8, dims=(2, 2, 2))
        rc = grp.solve_scene(sc, p)
        missing = set()
        for r, s in enumerate(grp.ranks):
            d, m = arrays(s)
            missing.update(m)
            np.savez(os.path.join(out, "%s_rank%d.npz" % (name, r)), **d)
        d = dict(rc=np.int32(rc), solveData=np.array(grp.stats.solveData[:], np.float64))
        for a in range(3):
            d["vel" + "XYZ"[a]], d["valid" + "XYZ"[a]] = grp.vel[a], grp.valid[a]
        np.savez(os.path.join(out, name + "_merged.npz"), **d)
        print("%-22s rc %d iterations %d origin of the last rank %s missing on any rank %s" % (
            name, rc, int(d["solveData"][1]), grp.bricks[-1].origin, sorted(missing)), flush=True)
        grp.close()

    single("a_blob", *jacobi(scenes.blob()))
    single("b_blob_pad1", *jacobi(scenes.blob(pad=1)))
    sc, p = jacobi(scenes.cavity(32, tile=8))
    p.doTile = 0
    single("c_cavity_one_region", sc, p)
    sc, p = jacobi(scenes.spheres(32, tile=8))
    single("d_spheres_density", scenes.with_density_field(sc, "layers"), p)
    single("e_droplet_sigma", *jacobi(scenes.ellipsoid_droplet(32, sigma=1.0)))
    bricks("f_bricks", *jacobi(scenes.cavity(32, tile=8)))
    sc, p = jacobi(scenes.cavity(32, tile=8))
    p.solverType = abi.EIGEN
    single("g_cavity_eigen_export", sc, p, export=True)
    # (f's ranks all see the whole 32^3 grid: the halo block is 16 cells.  Here the upper ranks start at global cell 16: gOff != 0.)
    bricks("h_bricks64", *jacobi(scenes.cavity(64, tile=8)))
    print("CASES DONE", flush=True)
    return 0


if __name__ == "__main__":
    argv = sys.argv[1:]
    if not argv or argv[0].startswith("-"):
        sys.exit(__doc__)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main(argv[0], os.path.abspath(argv[2]) if len(argv) == 3 and argv[1] == "--root" else here))

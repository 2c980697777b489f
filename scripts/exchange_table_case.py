#!/usr/bin/env python3
"""The 2 x 2 x 2 bricks of cavity64 as an in-process group, dumped to OUT/rank<r>.npz and OUT/merged.npz: every rank's solutionVector, owned
face masks and ps_dist_stats entries 0, 1, 2 and 7, the merged velocities and valid masks, result, error and iterations.  Run it on two
checkouts (--root) with the same switches (none, PS_FUSED_R=1 PS_DIST_OVERLAP=1, PS_DIST_FORWARD=1: read once per process), then
`solve_stages_cases.py --compare A B` says whether every array is identical byte for byte (profiles/exchange_table.md).
usage: exchange_table_case.py OUT [--root CHECKOUT]"""
import os, sys


def main(out, root):
    sys.path.insert(0, root)
    import numpy as np
    import polystokes_amd
    from polystokes_amd import scenes
    os.makedirs(out, exist_ok=True)
    sc, p = scenes.cavity(64, tile=16)
    grp = polystokes_amd.Group(8, dims=(2, 2, 2))
    rc = grp.solve_scene(sc, p)
    for r, s in enumerate(grp.ranks):
        st = s.dist_stats()
        d = dict(solutionVector=np.asarray(s.array("solutionVector")).copy(),
                 distStats=np.array([st["halo_bytes_per_iter"], st["owned_dofs"], float(st["overlap"]), st["halo_label_changes"]], np.float64))
        for a in "XYZ":
            d["owned" + a] = np.asarray(s.array("owned" + a)).copy()
        np.savez(os.path.join(out, "rank%d.npz" % r), **d)
    d = dict(rc=np.int32(rc), solveData=np.array(grp.stats.solveData[:], np.float64))
    for a in range(3):
        d["vel" + "XYZ"[a]], d["valid" + "XYZ"[a]] = grp.vel[a], grp.valid[a]
    np.savez(os.path.join(out, "merged.npz"), **d)
    st = grp.ranks[0].dist_stats()
    print("rc %d iterations %d error %.17g fused %d overlap %d bytes/iter rank 0 %d" % (
        rc, int(d["solveData"][1]), d["solveData"][0], int(grp.ranks[0].array("fusedStep")[0]), int(st["overlap"]), int(st["halo_bytes_per_iter"])), flush=True)
    grp.close()
    return 0


if __name__ == "__main__":
    argv = sys.argv[1:]
    if not argv or argv[0].startswith("-"):
        sys.exit(__doc__)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main(argv[0], os.path.abspath(argv[2]) if len(argv) == 3 and argv[1] == "--root" else here))

#!/usr/bin/env python3
"""The paths of the single-domain PCG solve (ps_context::solve) as twelve small cases in ONE process, each dumped to OUT/<case>.npz: every step
form, the polynomial in fp64 / fp32 / one term, the mixed-precision passes, warm starts, the budget running out into BiCGStab, an interrupt at
the first batch boundary.  Run it on two checkouts (--root) under `rocprofv3 --kernel-trace -- python3 ...`, once plain and once with
PS_FUSED_R=1 (the switch is read once per process), then compare: `--compare A B` says whether every array of every case is identical byte
for byte (of solveData the error and the iterations: the rest are times), `--compare-traces A.csv B.csv` whether the two kernel traces hold the same (kernel, grid, workgroup) line for line
(profiles/solve_stages.md).
usage: solve_stages_cases.py OUT [--root CHECKOUT] | --compare DIR_A DIR_B | --compare-traces A_kernel_trace.csv B_kernel_trace.csv"""
import csv, os, sys

ARRAYS = ("solutionVector", "fusedStep", "launchWalk", "solvePrecisionUsed", "solvePassIterations", "solveTrueResidual")


def compare(a, b):
    import numpy as np
    bad = 0
    names = sorted(set(os.listdir(a)) | set(os.listdir(b)))
    for f in names:
        if not (os.path.exists(os.path.join(a, f)) and os.path.exists(os.path.join(b, f))):
            print("MISSING", f); bad += 1
            continue
        za, zb = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        data = lambda z, k: z[k][:2] if k == "solveData" else z[k]      # solveData: error, iterations; then four times
        diff = [k for k in sorted(set(za.files) | set(zb.files))
                if k not in za.files or k not in zb.files or za[k].dtype != zb[k].dtype or data(za, k).tobytes() != data(zb, k).tobytes()]
        print("%-28s %s" % (f, "identical (%d arrays)" % len(za.files) if not diff else "DIFFERENT: " + ", ".join(diff)))
        bad += bool(diff)
    print("RESULT", "identical" if not bad and names else "different", len(names), "files")
    return 1 if bad or not names else 0


def trace_rows(path):
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))      # one stream: the order of the launches
    cols = ["Kernel_Name"] + [c for c in rows[0] if c.startswith(("Grid_Size", "Workgroup_Size"))] if rows else []
    assert not rows or len(cols) > 1, "no grid / workgroup columns in " + path
    return [tuple(r[c] for c in cols) for r in rows]


def compare_traces(a, b):
    ra, rb = trace_rows(a), trace_rows(b)
    first = next((i for i, (x, y) in enumerate(zip(ra, rb)) if x != y), None)
    if first is None and len(ra) != len(rb):
        first = min(len(ra), len(rb))
    print("launches", len(ra), len(rb), "distinct kernels", len(set(r[0] for r in ra)), len(set(r[0] for r in rb)))
    if first is not None:
        print("FIRST DIFFERENCE at launch", first, ra[first:first + 1], rb[first:first + 1])
    print("RESULT", "identical" if first is None and ra else "different")
    return 0 if first is None and ra else 1


def main(out, root):
    sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
    import numpy as np
    import polystokes_amd
    from polystokes_amd import scenes, _abi as abi
    import helpers
    os.makedirs(out, exist_ok=True)
    cavity = lambda: scenes.cavity(32)
    spheres = lambda: scenes.spheres(32, tile=8)

    def dump(name, s, rc):
        d = dict(rc=np.int32(rc), solveData=np.array(s.stats.solveData[:], np.float64), usedBiCGStab=np.int32(s.stats.usedBiCGStab))
        for a in ARRAYS:
            try:
                d[a] = np.asarray(s.array(a)).copy()
            except KeyError:                      # (the pass arrays exist after a mixed solve only)
                d[a] = np.zeros(0)
        np.savez(os.path.join(out, name + ".npz"), **d)
        print("%-24s rc %d iterations %d bicgstab %d fused %d used %d passes %s" % (
            name, rc, int(d["solveData"][1]), int(d["usedBiCGStab"]), int(d["fusedStep"][0]), int(d["solvePrecisionUsed"][0]),
            list(d["solvePassIterations"])), flush=True)

    def run(name, make, pre, degree=0, tol=1e-6, mixed=False, warm=False, maxit=20000, interrupt=False):
        sc, p = make()
        p.preconditioner, p.preconditionerDegree, p.tolerance, p.maxSolverIterations = pre, degree, tol, maxit
        s = polystokes_amd.Solver(0)
        try:
            assert s.set_solve_precision(abi.PRECISION_MIXED if mixed else abi.PRECISION_FP64) == abi.SUCCESS
            if warm:
                s.set_warm_start(abi.WARM_PREVIOUS_STEP)
            if interrupt:
                helpers.iterate_after(s, 1, sc, p)
                dump(name, s, abi.INCOMPLETE)
                return
            s.upload(sc, p)
            rc = s.step_device()
            if warm:
                dump(name + "_step1", s, rc)
                rc = s.step_device()
                assert int(s.array("warmStartUsed")[0]) == 1
            dump(name, s, rc)
        finally:
            s.close()

    run("a_jacobi", cavity, abi.PRE_DIAGONAL)
    run("b_identity", cavity, abi.PRE_IDENTITY)
    run("c_chebyshev4", cavity, abi.PRE_CHEBYSHEV, degree=4)
    run("d_chebyshev4_f32", cavity, abi.PRE_CHEBYSHEV_F32, degree=4)
    run("e_chebyshev1", cavity, abi.PRE_CHEBYSHEV, degree=1)
    run("f_mixed_1e-8", cavity, abi.PRE_DIAGONAL, tol=1e-8, mixed=True)
    for tag, make in (("cavity", cavity), ("spheres", spheres)):
        run("g_warm_" + tag, make, abi.PRE_DIAGONAL, warm=True)
        run("h_mixed_warm_" + tag, make, abi.PRE_DIAGONAL, mixed=True, warm=True)
    run("i_budget", cavity, abi.PRE_DIAGONAL, tol=1e-10, maxit=30)
    run("j_mixed_budget", cavity, abi.PRE_DIAGONAL, tol=1e-10, maxit=30, mixed=True)
    run("k_interrupt", cavity, abi.PRE_DIAGONAL, interrupt=True)
    run("l_mixed_interrupt", cavity, abi.PRE_DIAGONAL, mixed=True, interrupt=True)
    print("CASES DONE", flush=True)
    return 0


if __name__ == "__main__":
    argv = sys.argv[1:]
    if len(argv) == 3 and argv[0] == "--compare":
        sys.exit(compare(argv[1], argv[2]))
    if len(argv) == 3 and argv[0] == "--compare-traces":
        sys.exit(compare_traces(argv[1], argv[2]))
    if not argv or argv[0].startswith("-"):
        sys.exit(__doc__)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main(argv[0], os.path.abspath(argv[2]) if len(argv) == 3 and argv[1] == "--root" else here))

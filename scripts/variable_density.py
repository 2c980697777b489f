"""Per-iteration cost of a density FIELD (ps_upload_density_field: McInv then takes > 256 values and is not value-set coded) against the same
scene with a scalar density, on the cavity.  Each case runs in its own child process (PS_S_DUAL is read once per process), the cases
alternate round by round.  Cases: scalar / field with the one-unit S kernel (PS_S_DUAL=0) / field with the two-unit S kernel on the fp64
face mass (k_spmv_S_ell2u), Jacobi; then the fp32 Chebyshev polynomial on the scalar and the field scene.
usage: variable_density.py [res] [rounds]"""
import json, os, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def child(n, field, pre):
    import polystokes_amd
    from polystokes_amd import scenes, _abi as abi
    sc, p = scenes.cavity(n)
    sc.density = 4.0
    if field:
        scenes.with_density_field(sc, "smooth", rho0=4.0)
    p.preconditioner = {"jacobi": abi.PRE_DIAGONAL, "cheb32": abi.PRE_CHEBYSHEV_F32}[pre]
    s = polystokes_amd.Solver(0)
    s.upload(sc, p)
    s.step_device()                                   # warm-up step
    t0 = time.perf_counter()
    rc = s.step_device()
    ms = (time.perf_counter() - t0) * 1e3
    it = int(s.stats.solveData[1])
    print(json.dumps(dict(rc=rc, it=it, step_ms=ms, solve_ms=s.stats.stage_ms[8], us_per_it=s.stats.stage_ms[8] * 1e3 / max(it, 1),
                          dc=int(s.array("diagonalsCoded")[0]), c32=int(s.array("chebInner32")[0]), df=int(s.array("densityField")[0]))))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:
        child(int(sys.argv[2]), sys.argv[3] == "1", sys.argv[4])
        sys.exit(0)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    cases = [("a scalar", "0", "jacobi", {}), ("b field, one-unit S", "1", "jacobi", {"PS_S_DUAL": "0"}), ("c field, two-unit S", "1", "jacobi", {}),
             ("scalar cheb32", "0", "cheb32", {}), ("field cheb32", "1", "cheb32", {})]
    for r in range(rounds):
        for name, field, pre, env in cases:
            pr = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", str(n), field, pre],
                                capture_output=True, text=True, env=dict(os.environ, **env))
            if pr.returncode != 0:
                print("%s: child failed rc %d\n%s" % (name, pr.returncode, pr.stderr[-2000:]), flush=True)
                sys.exit(1)
            d = json.loads(pr.stdout.strip().splitlines()[-1])
            print("round %d cavity %d^3 %-22s rc %d it %4d step %8.1f ms solve %8.1f ms %7.1f us/it diagonalsCoded %d chebInner32 %d densityField %d" % (
                r, n, name, d["rc"], d["it"], d["step_ms"], d["solve_ms"], d["us_per_it"], d["dc"], d["c32"], d["df"]), flush=True)

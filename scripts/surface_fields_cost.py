"""Setup cost of the free-surface fields (ps_upload_surface_fields) for profiles/surface_fields.md: stage_ms of the setup on the 256^3 droplet
and the 256^3 cavity in three cases — no surface tension, a scalar sigma, both fields — each in its own child process, the cases alternating
round by round.  With --parent DIR (a checkout of the parent commit with its library built) the first two cases also run on the parent,
interleaved with this tree's: they run no changed code and must sit inside the parent's own spread.
usage: surface_fields_cost.py [--parent DIR] [res] [rounds]"""
import json, os, subprocess, sys
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(root, scene, case, n):
    sys.path.insert(0, root)
    import numpy as np
    import polystokes_amd
    from polystokes_amd import scenes, _abi as abi
    sc, p = scenes.droplet(n, tile=16) if scene == "droplet" else scenes.cavity(n)
    s = polystokes_amd.Solver(0)
    s.set_surface_tension(1.0 if case == "scalar" else 0.0)
    s.upload(sc, p)
    if case == "fields":
        rng = np.random.RandomState(11)
        sh = (sc.nz, sc.ny, sc.nx)
        assert s.upload_surface_fields(rng.uniform(0, 2, sh).astype(np.float32), rng.uniform(-500, 500, sh).astype(np.float32)) == abi.SUCCESS
    s.setup()                                         # warm-up: the buffers are allocated here
    out = []
    for _ in range(3):
        s.setup()
        st = [s.stats.stage_ms[q] for q in range(8)]
        out.append(dict(setup_ms=sum(st), assemble_ms=st[abi.STAGE_NAMES.index("assemble")]))
    best = min(out, key=lambda d: d["setup_ms"])
    names = ("surfaceFields",) if case == "fields" else ()
    print(json.dumps(dict(best, fields=[int(s.array(k)[0]) for k in names], sigma=float(s.array("surfaceTension")[0]))))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:
        child(sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5]))
        sys.exit(0)
    args = sys.argv[1:]
    parent = None
    if args[:1] == ["--parent"]:
        parent, args = os.path.abspath(args[1]), args[2:]
    n = int(args[0]) if args else 256
    rounds = int(args[1]) if len(args) > 1 else 3
    runs = []
    for case in ("none", "scalar"):
        if parent:
            runs.append(("parent", parent, case))
        runs.append(("this", HERE, case))
    runs.append(("this", HERE, "fields"))
    for scene in ("droplet", "cavity"):
        for r in range(rounds):
            for who, root, case in runs:
                pr = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", root, scene, case, str(n)],
                                    capture_output=True, text=True)
                if pr.returncode != 0:
                    print("%s %s %s: child failed rc %d\n%s" % (scene, who, case, pr.returncode, pr.stderr[-2000:]), flush=True)
                    sys.exit(1)
                d = json.loads(pr.stdout.strip().splitlines()[-1])
                print("round %d %s %d^3 %-6s %-6s setup %8.3f ms  assemble stage %7.3f ms  sigma %g fields %s" % (
                    r, scene, n, who, case, d["setup_ms"], d["assemble_ms"], d["sigma"], d["fields"]), flush=True)

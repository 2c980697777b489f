"""The PCG iterate after exactly 25 and 50 iterations against a plain fp64 restatement (helpers.numpy_pcg, fsum dot products) on the oracle's
operator and preconditioner.

A converged answer cannot see a wrong step kernel: PCG corrects itself and only takes a few more iterations.  The iterate after a fixed number
of iterations can: an interrupt (ps_set_interrupt) stops the solve at the m-th batch boundary, where solutionVector holds x after 25 m
iterations.  x_50 crosses one batch boundary, where the parity of the double-buffered scalars (CG_BATCH = 25 is odd) flips.

The decomposed solve (Dist::solve: slabs and bricks) is held to the same reference of the whole, uncut scene (section 3): one rank asks to
stop, every rank returns PS_INCOMPLETE at the same batch with x after 25 m updates on its owned DOFs (halo entries may be stale), and the
owned DOFs of all ranks merge into one x in the single domain's numbering (helpers.merged_x).  One process per rank:
test_gpu_multiprocess.py::test_multiprocess_iterates_match_the_reference.

Bounds: ITERATE_BOUND (fp64 steps) and ITERATE_BOUND_F32 (the fp32 Chebyshev polynomial, its M taken from the device) in helpers.py, measured on
an MI355X and checked against two perturbations of the reference itself by test_iterate_tolerances_cpu.py."""
import json
import os

import numpy as np
import pytest

from polystokes_amd import _abi as abi
from polystokes_amd import scenes

import children
import mp_cases
from helpers import (CG_BATCH, ITERATE_BOUND, ITERATE_BOUND_F32, ITERATE_DROPPED, ITERATE_SHORT, RANK_ARRAYS, SavedRanks, dof_numbering,
                     group_interrupted_step, group_iterate_after, iterate_after, make_parts, merged_x, numpy_pcg, relerr, trajectory_params)

pytestmark = pytest.mark.gpu


SCENES = {
    "cavity32": lambda: scenes.cavity(32),
    "coil32": lambda: scenes.coil(32, tile=8),
    "spheres32": lambda: scenes.spheres(32, tile=8),
    "blob6": lambda: scenes.blob(seed=6),                  # a viscosity field
    # the decomposed cases (section 3): the smallest that can be cut (partition.alignment is 16 for tiles 8 and 16) besides the three 32^3 above
    "blob32": lambda: scenes.blob(32, 32, 32, seed=6, tile=8),                  # a viscosity field: the fp64 stress diagonal
    "tall24x48": lambda: mp_cases.tall_cavity(24, 48, tile=8),                  # three slabs of 16 layers
    "tall32x64": lambda: mp_cases.tall_cavity(32, 64),                          # mp_cases' cavity_w2 and cavity_b2x1x2 (tile 16): one process per rank
    # the walk-forcing sets: S and St have more than 224 pairs of chunks (301 and 537 on spheres48), so that on a grid of 64 the runs of
    # 32 pairs dealt to every XCD hold chunks for every workgroup (coil48's S has 152 pairs: XCDs 5-7 would get none)
    "cavity48": lambda: scenes.cavity(48, tile=8),
    "coil48": lambda: scenes.coil(48, tile=8),
    "spheres48": lambda: scenes.spheres(48, tile=8),
    # the vector kernels' scalar tails (test_gpu_vector_tails.py): nSystem % 4 = 1, 2, 3 (viscosity fields: the fp64 stress diagonal) and 1 (the coded one)
    "tail1": lambda: scenes.blob(20, 18, 22, seed=4, tile=8),
    "tail2": lambda: scenes.blob(20, 18, 22, seed=1, tile=8),
    "tail3": lambda: scenes.blob(20, 18, 22, seed=2, tile=8),
    "tail1c": lambda: scenes.coil(30, tile=8),
}
PRECONDS = {"identity": (abi.PRE_IDENTITY, 0), "jacobi": (abi.PRE_DIAGONAL, 0), "cheb1": (abi.PRE_CHEBYSHEV, 1), "cheb2": (abi.PRE_CHEBYSHEV, 2),
            "cheb4": (abi.PRE_CHEBYSHEV, 4), "cheb10": (abi.PRE_CHEBYSHEV, 10), "cheb32": (abi.PRE_CHEBYSHEV_F32, 4)}


def make_case(scene, pre):
    sc, p = SCENES[scene]()
    p.preconditioner, deg = PRECONDS[pre]
    if deg:
        p.preconditionerDegree = deg
    return sc, p


def _identity(r):
    return np.array(r, copy=True)


def run_case(scene, pre, batches=None, ops=False):
    """One single-domain case on a fresh context: the device iterates after 25 m iterations (m in batches) against the reference.
    Returns {"drift": {iterations: relerr}, "fused", "apply", "precondition" (ops: full-vector relative errors against the oracle),
    "walk" (the launchWalk records of the last solve)}."""
    import polystokes_amd
    from oracle import ps_oracle
    sc, p = make_case(scene, pre)
    if batches is None:
        batches = ITERATE_SHORT.get((scene, pre), (1, 2))
    gpu = polystokes_amd.Solver(0)
    try:
        got = {CG_BATCH * m: iterate_after(gpu, m, sc, p) for m in batches}
        out = {"fused": int(gpu.array("fusedStep")[0]), "walk": gpu.array("launchWalk").reshape(5, 8).tolist()}
        b = gpu.array("b")
        n = len(b)
        o = ps_oracle.Oracle()
        o.run(sc, trajectory_params(p), solve=False)
        A, M = o.apply, o.precondition
        if ops:
            rng = np.random.RandomState(5)
            w = rng.standard_normal(n)
            out["apply"] = relerr(gpu.apply(w), o.apply(w))
            r = rng.standard_normal(n)
            out["precondition"] = relerr(gpu.precondition(r), o.precondition(r))
        if pre == "identity":
            M = _identity
        elif pre == "cheb32":
            M = gpu.precondition            # the fp32 polynomial as the device applies it (test_gpu_parity: 5e-6 of the oracle's)
        ref = {}
        numpy_pcg(A, M, b, np.zeros(n), 0.0, 0, iters=max(got),
                  on_iterate=lambda k, x: ref.__setitem__(k, x.copy()) if k in got else None)
        out["drift"] = {k: relerr(got[k], ref[k]) for k in got}
        return out
    finally:
        gpu.close()


def bound(pre):
    return ITERATE_BOUND_F32 if pre == "cheb32" else ITERATE_BOUND


def check(out, pre):
    for k, d in out["drift"].items():
        assert d <= bound(pre), (k, d, bound(pre))


# ---- 1. single domain, default forms ------------------------------------------------------------------------------------------------
SINGLE = [(scene, pre) for scene in ("cavity32", "coil32", "spheres32", "blob6") for pre in PRECONDS if (scene, pre) not in ITERATE_DROPPED]


@pytest.mark.parametrize("scene,pre", SINGLE)
def test_iterates_match_the_reference(scene, pre):
    """x_25 and x_50 of the default step forms against the fp64 reference.  Measured max |dx| / max |x| on an MI355X (x_25 / x_50):
      cavity32  identity 5.1e-15 / 1.3e-14, Jacobi 7.5e-15 / 2.5e-14, Chebyshev-1 4.0e-15 / 1.2e-14, -2 9.7e-15 / 1.3e-14, -4 5.4e-15 / 5.5e-15,
                -10 6.9e-15, fp32 1.0e-9 / 2.7e-11
      coil32    identity 4.2e-15 / 1.1e-14, Jacobi 4.2e-15 / 6.0e-15, Chebyshev-1 6.2e-15 / 7.7e-15, -2 2.9e-15 / 2.9e-15, -4 8.9e-16 / 8.9e-16,
                -10 1.0e-15, fp32 2.3e-10 / 2.4e-10
      spheres32 identity 1.8e-15 / 4.5e-15, Jacobi 5.1e-15 / 4.1e-15, Chebyshev-1 4.1e-15 / 5.8e-15, -2 8.4e-14 / 4.5e-14, -4 5.2e-14 / 3.8e-14,
                -10 6.5e-14 / 1.3e-13, fp32 1.4e-8 / 4.1e-9
      blob6     identity 1.6e-15 / 5.6e-15, Jacobi 1.6e-15 / 2.7e-15, Chebyshev-1 9.2e-16 / 3.2e-15, -2 8.0e-16 / 8.0e-16, -4 1.0e-15,
                fp32 1.3e-11 / 2.6e-14
    The fp32 polynomial's bound cannot see a 1e-6 error of beta (it moves x by 8e-11 to 1.4e-7): a known gap, its self-check is the zeroed
    row only."""
    check(run_case(scene, pre), pre)


# ---- 2. forced forms, one child process per switch set --------------------------------------------------------------------------------
_CHILD = (
    "import test_gpu_iterates as t\n"
    "out = []\n"
    "for case in json.loads(sys.argv[1]):\n"
    "    r = t.run_case(case[0], case[1], ops=True)\n"
    "    r['case'] = case\n"
    "    out.append(r)\n"
    "print('RESULT ' + json.dumps(out))\n"
)


def run_child(env, cases, timeout=900):
    return children.run_python(_CHILD, json.dumps(cases), limit=timeout, env=env).result()


_PAIR = [["coil32", "jacobi"], ["spheres32", "cheb4"]]
FORCED = {
    "fused_r": ({"PS_FUSED_R": "1"}, [["cavity32", q] for q in PRECONDS] + [["coil32", "jacobi"], ["spheres32", "cheb32"]]),
    "nt_level2": ({"PS_NT_LEVEL": "2"}, _PAIR),
    "one_unit": ({"PS_S_DUAL": "0", "PS_ST_DUAL": "0"}, _PAIR + [["blob6", "identity"]]),
    "no_ell": ({"PS_NO_ELL": "1"}, _PAIR),
    "one_shot": ({"PS_PIPE_GRID": "0"}, _PAIR),
    "fp64_values": ({"PS_FORCE_FP64_VALUES": "1"}, _PAIR),
    "tile_split_valu": ({"PS_TILE_SPLIT": "1", "PS_TILE_VALU": "1"}, _PAIR),
    # walks: grids far below the chunk count (multiples of 8: the XCD walk and the fp32 polynomial stay on).  The two-unit kernels deal runs
    # of 32 pairs to the XCDs whatever PS_XCD says; the one-unit kernels' runs follow PS_XCD (1: one chunk, 3: rounded down to 2) and
    # PS_WG_RUN (log2 of the consecutive chunks a workgroup takes)
    "walk_grid": ({"PS_PIPE_GRID": "64", "PS_PIPE_GRID_ST": "40", "PS_XCD": "1"},
                  [["spheres48", "jacobi"], ["spheres48", "cheb4"], ["cavity48", "cheb32"]]),
    "walk_grid_fused": ({"PS_PIPE_GRID": "64", "PS_PIPE_GRID_ST": "24", "PS_XCD": "1", "PS_FUSED_R": "1"},
                        [["spheres48", "jacobi"], ["spheres48", "cheb4"], ["cavity48", "cheb32"]]),
    "walk_xcd3_run0": ({"PS_PIPE_GRID": "64", "PS_XCD": "3", "PS_WG_RUN": "0", "PS_S_DUAL": "0", "PS_ST_DUAL": "0"},
                       [["coil48", "jacobi"], ["spheres48", "identity"]]),
    "walk_run2": ({"PS_PIPE_GRID": "48", "PS_XCD": "1", "PS_WG_RUN": "2", "PS_S_DUAL": "0", "PS_ST_DUAL": "0", "PS_FUSED_R": "1"},
                  [["cavity48", "jacobi"], ["spheres48", "identity"]]),
}
WALK_SETS = {"walk_grid", "walk_grid_fused", "walk_xcd3_run0", "walk_run2"}


def walk_records(walk):
    return [w for w in walk if w[0] == 1]


@pytest.mark.parametrize("name", list(FORCED))
def test_forced_forms_match_the_reference(name):
    """each switch set in its own process (the switches are read once per process): x_25 / x_50 against the reference, apply(x) against the
    oracle to 1e-12 of max |y|, precondition(r) to 1e-10 (5e-6 for the fp32 polynomial).

    launchWalk counts the steps in which a workgroup gets a chunk.  Under the walk-forcing sets every workgroup of every persistent launch
    gets at least two, some workgroups get more than others (a partial last run), and where the two-unit kernels walk pairs some launch has
    an odd chunk count (a half-empty last pair: spheres48's St, 1073 chunks).  Measured on an MI355X (least / most steps): walk_grid
    spheres48 S 4 / 8, St 26 / 28 and 12 / 18 (Chebyshev term), cavity48 S 8 / 12, St 52 / 54 and 25 / 32; walk_grid_fused St 21 / 30 and
    42 / 54; walk_xcd3_run0 coil48 4 / 5 and 8 / 9, spheres48 9 / 10 and 16 / 17; walk_run2 cavity48 24 / 28 and 44 / 44, spheres48
    12 / 16 and 20 / 24.

    Measured drift (x_25, x_50), fp64 steps: fused_r cavity32 every preconditioner 5.1e-15 .. 3.2e-14, coil32 Jacobi 5.6e-15 / 6.9e-15;
    nt_level2, one_unit, no_ell, one_shot, fp64_values: coil32 Jacobi 4.2e-15 .. 7.2e-15, spheres32 Chebyshev-4 2.8e-14 .. 5.3e-14, blob6
    identity 1.6e-15 / 5.6e-15; tile_split_valu coil32 1.4e-14 / 1.8e-14; the walk sets 1.5e-15 .. 5.1e-14.  fp32 polynomial: fused_r
    cavity32 1.3e-9 / 2.1e-11, spheres32 9.5e-9 / 4.0e-9; walk sets cavity48 5.4e-9 .. 7.6e-9 / 3.3e-10 .. 5.3e-10."""
    env, cases = FORCED[name]
    res = run_child(env, cases)
    for r in res:
        pre = r["case"][1]
        check(r, pre)
        assert r["apply"] <= 1e-12, r
        assert r["precondition"] <= (5e-6 if pre == "cheb32" else 1e-10), r
        if env.get("PS_FUSED_R") == "1":
            assert r["fused"] == 1, r
    if name in WALK_SETS:
        ws = [w for r in res for w in walk_records(r["walk"]) if w[1] != 0]     # (kernel 0: the one-shot CSR launch of a mode without a walk)
        assert ws and all(w[6] >= 2 for w in ws), ws                        # every workgroup of every persistent launch got >= 2 chunks
        assert any(w[6] != w[7] for w in ws), ws                             # a partial last run
        if any(w[5] for w in ws):
            assert any(w[5] and w[2] % 2 == 1 for w in ws), ws               # a half-empty last pair


# ---- 3. decomposed solves: in-process groups of slabs and bricks ---------------------------------------------------------------------------------
# The reference is that of the whole, uncut scene: the oracle's b, operator and preconditioner, x_0 = 0.  One per (scene, preconditioner),
# shared by every decomposition and every forced form of it, and never written to.
DECOMPS = {"slabs2": (2, None), "slabs3": (3, None), "b2x2x2": (8, (2, 2, 2)), "b2x1x2": (4, (2, 1, 2)), "b1x2x1": (2, (1, 2, 1))}
GROUP_CASES = [("slabs2", "cavity32", "identity"), ("slabs2", "cavity32", "jacobi"), ("slabs2", "cavity32", "cheb4"), ("slabs2", "coil32", "jacobi"),
               ("slabs2", "spheres32", "identity"), ("slabs2", "spheres32", "cheb4"), ("slabs2", "blob32", "jacobi"),
               ("slabs3", "tall24x48", "jacobi"), ("slabs3", "tall24x48", "cheb2"),
               ("b2x2x2", "spheres32", "jacobi"), ("b2x2x2", "spheres32", "cheb4"), ("b2x2x2", "cavity32", "identity"),
               ("b2x1x2", "coil32", "jacobi"), ("b1x2x1", "cavity32", "identity")]
_THREE = [["slabs2", "spheres32", "jacobi"], ["slabs3", "tall24x48", "jacobi"], ["b2x2x2", "spheres32", "cheb4"]]
_BRICKS = [["b2x2x2", "spheres32", "jacobi"], ["b2x1x2", "coil32", "jacobi"]]
GROUP_FORCED = {
    "fused_r": ({"PS_FUSED_R": "1"}, _THREE),
    "split": ({"PS_DIST_OVERLAP": "1"}, _THREE),
    "split_fused_r": ({"PS_DIST_OVERLAP": "1", "PS_FUSED_R": "1"}, _THREE),
    "forward": ({"PS_DIST_FORWARD": "1", "PS_FUSED_R": "0"}, _BRICKS),
    "forward_fused_r": ({"PS_DIST_FORWARD": "1", "PS_FUSED_R": "1"}, _BRICKS),
}
# test_gpu_multiprocess.py's iterate test, one process per rank: mp_cases' case -> the (scene, preconditioner) here
MP_CASES = {"cavity_w2": ("tall32x64", "identity"), "cavity_b2x1x2": ("tall32x64", "identity")}
_references = {}


def batches_of(scene, pre):
    return ITERATE_SHORT.get((scene, pre), (1, 2))


def reference(scene, pre):
    """({iterations: x of the fp64 restatement on the whole scene}, dof_numbering of the whole scene), computed once"""
    if (scene, pre) not in _references:
        from oracle import ps_oracle
        sc, p = make_case(scene, pre)
        o = ps_oracle.Oracle()
        o.run(sc, trajectory_params(p), solve=False)
        M = _identity if pre == "identity" else o.precondition
        b = o.array("b")
        ks = [CG_BATCH * m for m in batches_of(scene, pre)]
        ref = {}
        numpy_pcg(o.apply, M, b, np.zeros(len(b)), 0.0, 0, iters=max(ks), on_iterate=lambda k, x: ref.__setitem__(k, x.copy()) if k in ks else None)
        for x in ref.values():
            x.setflags(write=False)
        _references[(scene, pre)] = (ref, dof_numbering(o))
    return _references[(scene, pre)]


def group_forms(grp):
    """the step form every rank reports after a decomposed solve"""
    return {"fused": [int(r.array("fusedStep")[0]) for r in grp.ranks], "overlap": [int(bool(r.dist_stats()["overlap"])) for r in grp.ranks]}


def check_group(tag, scene, pre, got):
    """got: {iterations: merged x}"""
    ref, _ = reference(scene, pre)
    assert sorted(got) == sorted(ref)
    drift = {k: relerr(got[k], ref[k]) for k in sorted(got)}
    print("ITERATE %s %s %s " % (tag, scene, pre) + " / ".join("x_%d %.2e" % kd for kd in drift.items()))
    for k, d in drift.items():
        assert d <= ITERATE_BOUND, (tag, scene, pre, k, d, ITERATE_BOUND)


@pytest.mark.parametrize("decomp,scene,pre", GROUP_CASES)
def test_group_iterates_match_the_reference(decomp, scene, pre):
    """x_25 and x_50 of slabs and bricks in their default forms (the five-kernel step, one exchange round, the unsplit shared-stream
    launches), merged from the ranks' owned DOFs, against the reference of the whole scene: per-rank partial sums and the all-reduce of
    alpha and beta, the halo of p, the A p of rows on a cut, the preconditioner on a cut, the distributed Chebyshev interval and applies.
    The request to stop comes from the last rank alone; every rank must stop at the same batch.
    Measured max |dx| / max |x| on an MI355X (x_25 / x_50):
      slabs of 2    cavity32 identity 6.9e-15 / 2.2e-14, Jacobi 6.4e-15 / 1.8e-14, Chebyshev-4 5.2e-15 / 5.2e-15; coil32 Jacobi 3.8e-15 / 5.1e-15;
                    spheres32 identity 2.9e-15 / 6.6e-15, Chebyshev-4 5.2e-14 / 3.5e-14; blob32 Jacobi 1.4e-15 / 1.4e-15
      slabs of 3    tall24x48 Jacobi 5.8e-15 / 1.1e-14, Chebyshev-2 7.2e-15 / 7.6e-15
      2 x 2 x 2     spheres32 Jacobi 4.8e-15 / 4.1e-15, Chebyshev-4 5.2e-14 / 3.5e-14; cavity32 identity 4.2e-15 / 1.2e-14
      2 x 1 x 2     coil32 Jacobi 3.6e-15 / 4.6e-15
      1 x 2 x 1     cavity32 identity 4.5e-15 / 1.1e-14
    All within the spread of the single-domain forms (1e-15 to 1.3e-13), the Chebyshev cases included: the decomposition's interval estimate
    differs from the oracle's by a reduction order only, and ITERATE_BOUND holds for them as it stands."""
    import polystokes_amd
    world, dims = DECOMPS[decomp]
    sc, p = make_case(scene, pre)
    _, numbering = reference(scene, pre)
    got = {}
    for m in batches_of(scene, pre):
        grp = polystokes_amd.Group(world, dims=dims)
        try:
            got[CG_BATCH * m] = group_iterate_after(grp, m, sc, p, numbering=numbering)
            forms = group_forms(grp)
        finally:
            grp.close()
        assert forms["fused"] == [0] * world and forms["overlap"] == [0] * world, forms     # small systems: the default is the five-kernel step
    check_group(decomp, scene, pre, got)


def group_child(cases, outdir):
    """(in the child of a forced form) every case's interrupted solves on fresh groups; per case and iterate one npz with the arrays of
    RANK_ARRAYS of every rank ("r<rank>.<name>") and the forms the ranks report.  The parent merges and compares: it holds the references."""
    import polystokes_amd
    for decomp, scene, pre in cases:
        world, dims = DECOMPS[decomp]
        sc, p = make_case(scene, pre)
        for m in batches_of(scene, pre):
            grp = polystokes_amd.Group(world, dims=dims)
            try:
                group_interrupted_step(grp, m, sc, p)
                out = {"r%d.%s" % (q, nm): r.array(nm) for q, r in enumerate(grp.ranks) for nm in RANK_ARRAYS}
                out.update({k: np.array(v) for k, v in group_forms(grp).items()})
            finally:
                grp.close()
            np.savez(os.path.join(outdir, "%s.%s.%s.%d.npz" % (decomp, scene, pre, CG_BATCH * m)), **out)


_GROUP_CHILD = (
    "import test_gpu_iterates as t\n"
    "t.group_child(json.loads(sys.argv[1]), sys.argv[2])\n"
    "print('RESULT ' + json.dumps('done'))\n"
)


@pytest.mark.parametrize("name", list(GROUP_FORCED))
def test_group_forced_forms_match_the_reference(name, tmp_path):
    """The other forms of the decomposed step, each switch set in one child process: the four-kernel step across the cuts (PS_FUSED_R=1:
    k_dist_fixup, k_relay2), the split interior / boundary launches with pack, transport and unpack (PS_DIST_OVERLAP=1), both, and the three
    forwarding rounds (PS_DIST_FORWARD=1) under either step.  Every rank must report the form: fusedStep 1 under PS_FUSED_R=1, and overlap on
    where PS_DIST_OVERLAP=1 meets the four-kernel step.  Dist::chooseStepForm splits the launches of the four-kernel step only (overlap =
    fused && ...) and has no four-kernel step for the Chebyshev polynomial (fused = !cheb && ...): PS_DIST_OVERLAP=1 alone leaves systems
    this small (below FUSED_STEP_MIN_ROWS) on the unsplit five-kernel step, and the Chebyshev case runs five kernels under every set — there
    the ranks must report 0 for both, so that a change of either rule shows here.
    Measured max |dx| / max |x| on an MI355X (x_25 / x_50), slabs-2 spheres32 Jacobi; slabs-3 tall24x48 Jacobi; 2 x 2 x 2 spheres32 Chebyshev-4:
      fused_r          4.8e-15 / 4.1e-15; 5.3e-15 / 9.9e-15; 5.2e-14 / 3.5e-14
      split            4.8e-15 / 4.0e-15; 5.8e-15 / 1.1e-14; 5.2e-14 / 3.5e-14
      split_fused_r    4.9e-15 / 4.0e-15; 4.5e-15 / 7.7e-15; 5.2e-14 / 3.5e-14
    and 2 x 2 x 2 spheres32 Jacobi; 2 x 1 x 2 coil32 Jacobi:
      forward          4.8e-15 / 4.1e-15; 3.6e-15 / 4.6e-15
      forward_fused_r  5.6e-15 / 4.5e-15; 4.3e-15 / 5.2e-15"""
    env, cases = GROUP_FORCED[name]
    assert children.run_python(_GROUP_CHILD, json.dumps(cases), str(tmp_path), limit=60 + 40 * len(cases), env=env).result() == "done"
    for decomp, scene, pre in cases:
        world, dims = DECOMPS[decomp]
        sc, p = make_case(scene, pre)
        (_, (where, n)), parts = reference(scene, pre), make_parts(sc, p.tileSize, world, dims)
        got = {}
        for m in batches_of(scene, pre):
            k = CG_BATCH * m
            f = np.load(str(tmp_path / ("%s.%s.%s.%d.npz" % (decomp, scene, pre, k))))
            four = int(env.get("PS_FUSED_R") == "1" and not pre.startswith("cheb"))
            assert f["fused"].tolist() == [four] * world, (name, decomp, scene, pre, f["fused"])
            assert f["overlap"].tolist() == [int(four and env.get("PS_DIST_OVERLAP") == "1")] * world, (name, decomp, scene, pre, f["overlap"])
            saved = [{nm: f["r%d.%s" % (q, nm)] for nm in RANK_ARRAYS} for q in range(world)]
            got[k] = merged_x(where, n, SavedRanks(saved, parts, dims), sc)
        check_group(name + "/" + decomp, scene, pre, got)


def all_cases():
    """every (scene, preconditioner) whose iterates a test here or test_gpu_multiprocess.py's iterate test compares: the tolerance self-checks
    (test_iterate_tolerances_cpu.py) run on them"""
    return sorted(set(SINGLE) | {tuple(c) for _, cases in FORCED.values() for c in cases} | {(s, q) for _, s, q in GROUP_CASES}
                  | {(c[1], c[2]) for _, cases in GROUP_FORCED.values() for c in cases} | set(MP_CASES.values()))

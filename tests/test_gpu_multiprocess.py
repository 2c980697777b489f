"""The REAL multi-process distributed path on one GPU: one process per rank, each with its own ps_context holding a
slab, ps_step_device -> ps_dist_step_single, halos and scalars exchanged through the host-staged TCP transport
(ps_comm_init_tcp; RCCL refuses several ranks on one device).  Same Dist code as the RCCL path except transport()/
allreduce().  Compared with the single-domain solve of the whole scene."""
import json
import os
import sys

import numpy as np
import pytest

from polystokes_amd import _abi as abi
from polystokes_amd import partition

import children
import mp_cases

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _run_ranks(case, world, tmp_path, env=None, per_process=1, limit=240):
    """per_process > 1: every process holds that many ranks, one thread each (mp_rank.py) — the box admits six GPU processes"""
    base = children.free_port_base(world)
    outs = [str(tmp_path / f"{case}.r{r}.npz") for r in range(world)]
    groups = [list(range(q, min(q + per_process, world))) for q in range(0, world, per_process)]
    children.run_group([children.script_argv("mp_rank.py", case, world, ",".join(str(r) for r in g), base, ",".join(outs[r] for r in g)) for g in groups],
                       limit=limit, env=env)
    return [np.load(o) for o in outs]


@pytest.mark.parametrize("case", ["cavity_w2", "cavity_w3_jacobi", "coil_w2", "cavity_w2_bicgstab", "cavity_w2_chebyshev",
                                  "cavity_w2+fused", "cavity_w3_jacobi+fused", "coil_w2+fused", "cavity_w2_bicgstab+fused",
                                  "cavity64_b2x2x1", "cavity_b2x1x2+fused"])
def test_multiprocess_tcp_matches_single_domain(case, tmp_path):
    """"+fused": the four-kernel PCG step across the slabs (default from 1.2 M owned rows per rank), forced in the rank processes."""
    env = {"PS_FUSED_R": "1"} if case.endswith("+fused") else None
    case = case.replace("+fused", "")
    world = mp_cases.WORLD[case]
    res = _run_ranks(case, world, tmp_path, env)     # children first: the parent's own GPU context comes after
    if env:
        assert all(int(r["fused"]) == 1 for r in res)
    _compare_with_single_domain(case, world, res)


STUB_LIB = os.path.join(HERE, "stub_rccl", "libps_stub_rccl.so")


@pytest.mark.parametrize("case", ["cavity_w2+fused", "cavity_w3_jacobi+fused", "coil_w2+fused", "cavity64_b2x2x1+fused", "cavity_b2x1x2+fused",
                                  "cavity_w2", "cavity_w2_chebyshev", "cavity_w2_bicgstab+fused"])
def test_multiprocess_async_transport_matches_tcp_and_single_domain(case, tmp_path):
    """The ASYNCHRONOUS transport branch (Dist::transport / allreduce with useRccl: every send, receive and all-reduce enqueued on the
    comm stream, ordered against the solver stream by events only) with N > 1 ranks on ONE GPU: the rank processes load tests/stub_rccl
    in place of librccl (PS_RCCL_LIB) — messages are stream-ordered device copies through hipIpcMemHandle-mapped mailboxes, ordered
    across the processes by hipIpcEventHandle events, and nothing in it synchronises the host with the device.  (The TCP transport
    calls hipStreamSynchronize twice per exchange and the in-process group shares one stream: both hide a missing order().)
    Two processes as slabs, three as slabs, four as 2 x 2 x 1 and 2 x 1 x 2 bricks — the box admits 6 GPU processes, so the 2 x 2 x 2
    case stays with the in-process groups — overlapped four-kernel step and five-kernel step: the same result as the single domain
    and, bit for bit, as the run over TCP (same kernels, same reduction order)."""
    if not os.path.exists(STUB_LIB):
        pytest.fail("tests/stub_rccl/libps_stub_rccl.so is missing: __graft_entry__.build() compiles it")
    fused = case.endswith("+fused")
    case = case.replace("+fused", "")
    world = mp_cases.WORLD[case]
    env = {"PS_TEST_TRANSPORT": "stub", "PS_RCCL_LIB": STUB_LIB, "PS_DIST_OVERLAP": "1"}
    if fused:
        env["PS_FUSED_R"] = "1"
    res = _run_ranks(case, world, tmp_path, env)
    if fused:
        assert all(int(r["fused"]) == 1 for r in res)
        if "bicgstab" not in case:
            assert all(int(r["overlap"]) == 1 for r in res)        # the exchanges really ran under the rows that do not need them
    _compare_with_single_domain(case, world, res)
    (tmp_path / "tcp").mkdir()
    res_tcp = _run_ranks(case, world, tmp_path / "tcp", {"PS_FUSED_R": "1"} if fused else None)
    for r in range(world):
        assert int(res[r]["iters"]) == int(res_tcp[r]["iters"]) and int(res[r]["rc"]) == int(res_tcp[r]["rc"])
        for a in range(3):
            assert np.array_equal(res[r]["vel%d" % a], res_tcp[r]["vel%d" % a]), (case, r, a)


def test_eight_asynchronous_ranks_as_bricks(tmp_path):
    """2 x 2 x 2 bricks of a 32^3 cavity (tile 8) over the asynchronous transport: EIGHT ranks, every one with its own ps_context, solver stream and comm
    stream, exchanging with three face neighbours and three diagonal ones in one grouped round (Dist::valuesOut / contributionsBack) and
    all-reducing among eight — as four processes of two ranks (one thread each; tests/stub_rccl reaches a rank of the same process through
    its device pointer).  The overlapped four-kernel step, Jacobi-PCG; compared with the single domain.  (VERDICT r04 missing #3: eight
    asynchronous ranks had never run; the in-process group of eight shares one stream.)"""
    if not os.path.exists(STUB_LIB):
        pytest.fail("tests/stub_rccl/libps_stub_rccl.so is missing: __graft_entry__.build() compiles it")
    case, world = "cavity32_b2x2x2", 8           # tile 8, bricks of 16^3 owned cells (eight ranks share one GPU: the 64^3 case takes 50 s per run, this one 10)
    env = {"PS_TEST_TRANSPORT": "stub", "PS_RCCL_LIB": STUB_LIB, "PS_DIST_OVERLAP": "1", "PS_FUSED_R": "1"}
    res = _run_ranks(case, world, tmp_path, env, per_process=2)
    assert all(int(r["fused"]) == 1 and int(r["overlap"]) == 1 for r in res)
    _compare_with_single_domain(case, world, res)
    (tmp_path / "fwd").mkdir()                   # the three forwarding rounds of r03 / r04
    res_fwd = _run_ranks(case, world, tmp_path / "fwd", dict(env, PS_DIST_FORWARD="1"), per_process=2)
    _compare_with_single_domain(case, world, res_fwd)


def test_async_transport_exposes_a_missing_stream_order(tmp_path):
    """The point of the stand-in: with the event that makes the solver stream wait for the unpacked halo values removed
    (PS_DIST_SKIP_ORDER=1: Dist::order(c, 1, false)), the overlapped step over the asynchronous transport reads stale halo values and
    the solve goes wrong.  (Over TCP the host blocks in hipStreamSynchronize around every exchange, which can order the streams by accident.)"""
    case, world = "cavity_b2x1x2", 4
    base_env = {"PS_FUSED_R": "1", "PS_DIST_SKIP_ORDER": "1"}
    res = _run_ranks(case, world, tmp_path, dict(base_env, PS_TEST_TRANSPORT="stub", PS_RCCL_LIB=STUB_LIB))
    (tmp_path / "ok").mkdir()
    good = _run_ranks(case, world, tmp_path / "ok", {"PS_FUSED_R": "1", "PS_TEST_TRANSPORT": "stub", "PS_RCCL_LIB": STUB_LIB})
    differs = any(int(res[r]["rc"]) != int(good[r]["rc"]) or int(res[r]["iters"]) != int(good[r]["iters"]) or
                  (int(res[r]["rc"]) in (0, 1) and any(not np.array_equal(res[r]["vel%d" % a], good[r]["vel%d" % a]) for a in range(3))) for r in range(world))
    assert differs, "the solve without the stream ordering came out bit-identical: the transport hides the race"


def _compare_with_single_domain(case, world, res):
    import polystokes_amd
    sc, p = mp_cases.make(case)
    single = polystokes_amd.Solver(0)
    if mp_cases.colliders(case) is None:
        rc1 = single.step(sc, p)
    else:                                   # upload, place, paint, step, download: polystokes_step would upload over the placement
        single.upload(sc, p)
        mp_cases.place_and_paint(single, case)
        rc1 = single.step_device()
        single.download()
    assert all(int(r["rc"]) == rc1 for r in res), [(int(r["rc"]), str(r["err"])) for r in res]
    it1 = single.stats.solveData[1]
    assert all(abs(int(r["iters"]) - it1) <= max(2, 0.02 * it1) for r in res), (it1, [int(r["iters"]) for r in res])
    assert all(int(r["used_bicgstab"]) == single.stats.usedBiCGStab for r in res)
    lab = single.array("centerLabels").reshape(sc.nz, sc.ny, sc.nx)
    sh = abi.grid_shapes(sc.nx, sc.ny, sc.nz)
    vel = [np.array(sc.vel[a], copy=True) for a in range(3)]
    valid = [np.zeros(sh["face" + "XYZ"[a]], np.float32) for a in range(3)]
    dims = mp_cases.DIMS.get(case)
    for r in range(world):
        if dims is not None:            # bricks (ps_set_brick): the same checks on the owned box
            b = partition.make_brick((sc.nx, sc.ny, sc.nz), dims, r, p.tileSize)
            ll = res[r]["labels"].reshape(b.n_local[2], b.n_local[1], b.n_local[0])
            assert np.array_equal(ll[b.lo[2]:b.hi[2], b.lo[1]:b.hi[1], b.lo[0]:b.hi[0]], lab[b.g0[2]:b.g1[2], b.g0[1]:b.g1[1], b.g0[0]:b.g1[0]]), (case, r)
            for a in range(3):
                shp = (b.n_local[2] + (a == 2), b.n_local[1] + (a == 1), b.n_local[0] + (a == 0))
                partition.merge_faces_brick(vel[a], res[r]["vel%d" % a].reshape(shp), res[r]["owned%d" % a], b, a)
                partition.merge_faces_brick(valid[a], res[r]["valid%d" % a].reshape(shp), res[r]["owned%d" % a], b, a)
            continue
        sl = partition.make_slab(sc.nz, world, r, p.tileSize)
        ll = res[r]["labels"].reshape(sl.nz_local, sc.ny, sc.nx)
        assert np.array_equal(ll[sl.zLoOwned:sl.zHiOwned], lab[sl.z0:sl.z1]), (case, r)
        for a in range(3):
            partition.merge_faces(vel[a], res[r]["vel%d" % a], res[r]["owned%d" % a], sl, a)
            partition.merge_faces(valid[a], res[r]["valid%d" % a], res[r]["owned%d" % a], sl, a)
    for a in range(3):
        assert np.array_equal(valid[a], single.valid[a]), case
        if rc1 == abi.SUCCESS:
            scale = max(np.abs(single.vel[a]).max(), 1e-30)
            assert np.abs(vel[a] - single.vel[a]).max() <= 20 * p.tolerance * scale, case
    single.close()


def test_multiprocess_interrupt_stops_every_rank(tmp_path):
    """An interrupt callback on ONE rank: all ranks return PS_INCOMPLETE after the same batch, nobody hangs in a receive."""
    res = _run_ranks("cavity_w2_interrupt", 2, tmp_path)
    assert [int(r["rc"]) for r in res] == [abi.INCOMPLETE, abi.INCOMPLETE]
    assert int(res[0]["iters"]) == int(res[1]["iters"]) == 25


@pytest.mark.parametrize("case,transport", [("cavity_w2", "tcp"), ("cavity_w2", "stub"), ("cavity_w2+fused", "stub"), ("cavity_b2x1x2", "stub")])
def test_multiprocess_iterates_match_the_reference(case, transport, tmp_path):
    """x_25 and x_50 of the production path — one process per rank, a comm stream, events, asynchronous sends (the in-process groups of
    test_gpu_iterates.py share one stream) — against the same fp64 reference of the whole scene, to the same bound: two slabs over TCP, over
    the stand-in RCCL library with the five-kernel step and with the overlapped four-kernel step, and 2 x 1 x 2 bricks (four processes) over
    the stand-in.  Only the last rank asks to stop, at its m-th batch; every rank must report PS_INCOMPLETE after 25 m iterations.  The ranks
    save their solutionVector and index arrays (mp_rank.py, "_iterate<m>"); the merge is helpers.merged_x.
    Measured max |dx| / max |x| on an MI355X (x_25 / x_50): cavity_w2 over TCP 1.4e-14 / 4.5e-14, over the stand-in the same figures (same
    kernels, same reduction order), with the four-kernel step 7.0e-15 / 2.3e-14; cavity_b2x1x2 over the stand-in 9.1e-15 / 2.8e-14."""
    import test_gpu_iterates as ti
    from helpers import CG_BATCH, SavedRanks, make_parts, merged_x
    if transport == "stub" and not os.path.exists(STUB_LIB):
        pytest.fail("tests/stub_rccl/libps_stub_rccl.so is missing: __graft_entry__.build() compiles it")
    fused = case.endswith("+fused")
    case = case.replace("+fused", "")
    world, dims = mp_cases.WORLD[case], mp_cases.DIMS.get(case)
    env = {"PS_TEST_TRANSPORT": "stub", "PS_RCCL_LIB": STUB_LIB} if transport == "stub" else {}
    if fused:
        env["PS_FUSED_R"] = "1"
    scene, pre = ti.MP_CASES[case]
    sc, p = mp_cases.make(case)
    got = {}
    for m in ti.batches_of(scene, pre):       # children first: the parent opens no GPU context here at all
        (tmp_path / str(m)).mkdir()
        res = _run_ranks("%s_iterate%d" % (case, m), world, tmp_path / str(m), env, limit=120)
        assert [int(r["rc"]) for r in res] == [abi.INCOMPLETE] * world, [(int(r["rc"]), str(r["err"])) for r in res]
        assert [int(r["iters"]) for r in res] == [CG_BATCH * m] * world
        assert [int(r["calls"]) for r in res] == [0] * (world - 1) + [m]
        assert [int(r["fused"]) for r in res] == [int(fused)] * world and [int(r["overlap"]) for r in res] == [int(fused)] * world
        where, n = ti.reference(scene, pre)[1]
        got[CG_BATCH * m] = merged_x(where, n, SavedRanks(res, make_parts(sc, p.tileSize, world, dims), dims), sc)
    ti.check_group("%s/%s%s" % (case, transport, "+fused" if fused else ""), scene, pre, got)


def test_multiprocess_ranks_place_and_paint_colliders(tmp_path):
    """spheres64_w2_colliders: two rank processes over TCP, each placing three sphere volumes (one across the cut) and painting their
    motions on its own slab from its own orig before the step.  The merged velocities and valid flags against the single domain that
    places and paints the whole grid; and x_25 of every rank (the "_iterate1" form: the last rank stops the solve at the first batch)
    against the in-process group of the same case that does the same calls through Group.set_scene's hook, rank by rank, to ITERATE_BOUND:
    the two differ by the order of the all-reduce alone."""
    import polystokes_amd
    from helpers import CG_BATCH, DOF_KINDS, ITERATE_BOUND, SavedRanks, dof_field, merge_dof_field, relerr, trajectory_params
    case, world = "spheres64_w2_colliders", 2
    res = _run_ranks(case, world, tmp_path)            # children first: the parent's own GPU context comes after
    _compare_with_single_domain(case, world, res)
    (tmp_path / "it").mkdir()
    it = _run_ranks(case + "_iterate1", world, tmp_path / "it", limit=120)
    assert [int(r["rc"]) for r in it] == [abi.INCOMPLETE] * world, [(int(r["rc"]), str(r["err"])) for r in it]
    assert [int(r["iters"]) for r in it] == [CG_BATCH] * world
    sc, p = mp_cases.make(case)
    grp = polystokes_amd.Group(world)
    try:
        calls = []
        grp.set_scene(sc, trajectory_params(p), per_rank=lambda s, part, local: mp_cases.place_and_paint(s, case), when="before_cut")
        grp.ranks[-1].set_interrupt(lambda: calls.append(1) or len(calls) >= 1)
        try:
            rc = grp.step()
        finally:
            grp.ranks[-1].set_interrupt(None)
        assert rc == abi.INCOMPLETE and int(grp.stats.solveData[1]) == CG_BATCH
        saved = SavedRanks(it, grp.slabs, None).ranks
        for r, slab in enumerate(grp.slabs):               # the DOFs the rank owns (a halo entry may be stale on either side: nothing reads it)
            assert it[r]["solutionVector"].shape == grp.ranks[r].array("solutionVector").shape
            for kind in DOF_KINDS:
                got, want = (dof_field(q, kind, q.array("solutionVector"), np.float64) for q in (saved[r], grp.ranks[r]))
                own_got, own_want = np.full_like(got, np.nan), np.full_like(want, np.nan)
                one = type(slab)(slab.rank, slab.world, slab.z0, slab.z1, slab.lo_halo, slab.hi_halo)
                one.g0 = 0                                     # merge into an array of the rank's own layers
                merge_dof_field(own_got, got, one, kind)
                merge_dof_field(own_want, want, one, kind)
                assert np.array_equal(np.isnan(own_got), np.isnan(own_want)), (r, kind)
                m = ~np.isnan(own_want)
                d = relerr(own_got[m], own_want[m])
                print("rank", r, kind, "x_25 process against in-process group: %.2e over %d owned DOFs" % (d, int(m.sum())))
                assert m.any() and d <= ITERATE_BOUND, (r, kind, d)
    finally:
        grp.close()


def test_decomposed_step_does_not_report_an_earlier_fp32_polynomial(tmp_path):
    """Every rank's context first solves its local scene on its own with PS_PRE_CHEBYSHEV_F32 (the fp32 polynomial runs: array chebInner32
    reads 1), then set_slab, comm_init_tcp and a decomposed step, whose polynomial is fp64: the array must read 0 on every rank, not the
    value the single-domain solve left.  The decomposed result still matches the single domain."""
    res = _run_ranks("cavity_w2_chebyshev_f32first", 2, tmp_path)
    assert all(int(r["single_rc"]) in (abi.SUCCESS, abi.NOCONVERGE) and int(r["single_c32"]) == 1 for r in res)
    assert [int(r["c32"]) for r in res] == [0, 0]
    _compare_with_single_domain("cavity_w2_chebyshev", 2, res)


def test_multiprocess_list_mismatch_fails_every_rank(tmp_path):
    """Ranks that were handed different fields for the same cells (here: rank 1 sees air in a patch of its own first layers, rank 0's
    halo copy does not): rank 0 finds the owner's labels differing from its copy deeper inside the halo block than the classification
    reaches (Dist::exchangeLabels), and EVERY rank returns FAILED instead of solving on inconsistent data or waiting for ever.
    (Until r04 the halo labels were the rank's own and the same case was caught one step later, by the counts / key hashes of the
    exchange lists — that check is still there: `checkLists`.)"""
    res = _run_ranks("cavity_w2_failrank", 2, tmp_path)
    assert [int(r["rc"]) for r in res] == [-1, -1], [str(r["err"]) for r in res]
    assert all("labels of a halo block" in str(r["err"]) for r in res), [str(r["err"]) for r in res]
    assert "different fields" in str(res[0]["err"])


def test_multiprocess_tile_size_mismatch_fails_every_rank(tmp_path):
    """Rank 1 runs with tileSize 8 on a slab cut for rank 0's 16: both pass ps_set_slab (the cut at z = 32 and the 16-cell halo block suit
    either), cross-section and halo layers agree, so only the tile size in the key the ranks swap before the first label exchange differs
    (Dist::handshakeCuts).  EVERY rank returns FAILED with the handshake's message; nobody waits in a receive sized for the other's labels."""
    res = _run_ranks("cavity_w2_tilemismatch", 2, tmp_path)
    errs = [str(r["err"]) for r in res]
    assert [int(r["rc"]) for r in res] == [-1, -1], errs
    assert all("configured differently" in e or "another pair of ranks" in e for e in errs), errs
    assert any("configured differently" in e for e in errs), errs


def _bench_line(*args, limit, env=None):
    """bench.py in a child: its stdout must be ONE line of JSON"""
    pr = children.run([sys.executable, os.path.join(os.path.dirname(HERE), "bench.py")] + list(args), limit=limit, env=env)
    lines = [l for l in pr.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, pr.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_two_ranks_produces_one_line_whatever_the_transport(tmp_path):
    """`python bench.py --gpus 2 --full` without a launcher: spawns one process per rank, rendezvous over gloo, and prints ONE JSON
    line.  With two GPUs the ranks talk over RCCL; on a one-GPU box RCCL refuses the duplicate device, every rank agrees on that
    (gloo) before any further collective, and all of them switch to the host-staged transport — the line says which."""
    import polystokes_amd
    try:                                   # a second device?  (probed through the library: no torch import in this process)
        polystokes_amd.Solver(1).close()
        two_gpus = True
    except polystokes_amd.PolyStokesError:
        two_gpus = False
    d = _bench_line("--gpus", "2", "--res", "32", "--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline", "--strong-res", "96",
                    limit=420, env={"MASTER_PORT": str(children.free_port_base(1))})
    assert d["n_gpus"] == 2 and d["unit"] == "ms/step" and d["value"] > 0 and d["cg_iterations"] > 0
    assert d["config"]["grid"] == [32, 32, 64] and d["scaling"] == "weak"
    if two_gpus:
        assert d["transport"] == "rccl"
    else:
        assert d["transport"].startswith("tcp (FALLBACK")
    # the strong-scaling block of the same invocation (BASELINE config 4 at --strong-res: here the 96^3 coil in two slabs)
    sb = d["strong_512"]
    assert sb["n_gpus"] == 2 and sb["scaling"] == "strong" and sb["decomposition"] == "1x1x2 bricks" and sb["ms_per_step"] > 0 and sb["result"] == 1
    single = polystokes_amd.Solver(0)
    from polystokes_amd import scenes
    sc, p = scenes.coil(96)
    p.preconditioner = 5          # abi.PRE_DIAGONAL: bench.py's default --precond jacobi
    single.step(sc, p)
    assert abs(sb["cg_iterations"] - single.stats.solveData[1]) <= max(2, 0.02 * single.stats.solveData[1])
    single.close()


def test_bench_four_ranks_as_bricks(tmp_path):
    """`bench.py --gpus 4 --bricks 2x2x1`: the decomposition along x and y (ps_set_brick), weak scaling = 32^3 owned cells per rank of the
    64 x 64 x 32 cavity; on a one-GPU box over the host-staged transport."""
    d = _bench_line("--gpus", "4", "--bricks", "2x2x1", "--res", "32", "--steps", "1", "--warmup", "1", "--no-cpu-baseline", "--no-strong-512",
                    "--transport", "tcp", limit=420, env={"MASTER_PORT": str(children.free_port_base(1))})
    assert d["n_gpus"] == 4 and d["value"] > 0 and d["cg_iterations"] > 0
    assert d["config"]["grid"] == [64, 64, 32] and "2x2x1 bricks" in d["config"]["parallelism"]
    # the same system as one rank solves it: the iteration count of the 64 x 64 x 32 cavity
    import polystokes_amd
    from polystokes_amd import scenes, partition
    sc = abi.Scene(64, 64, 32, 1.0 / 32, 1.0e-2, 1.0, [np.pad(np.zeros((31, 64, 65), np.float32), ((0, 1), (0, 0), (0, 0)), constant_values=1.0), 0.0, 0.0], -1.0, 1.0, 1.0)
    _, p = scenes.cavity(32, tile=16, pad=2, precond=abi.PRE_DIAGONAL)
    single = polystokes_amd.Solver(0)
    assert single.step(sc, p) == abi.SUCCESS
    assert abs(single.stats.solveData[1] - d["cg_iterations"]) <= max(2, 0.02 * single.stats.solveData[1])
    single.close()


def test_rccl_communicator_next_to_a_live_torch_context():
    """bench.py's situation for N > 1: torch imported and its GPU context live, then the library's RCCL communicator.  The library
    must pick up the librccl torch has already mapped (RTLD_NOLOAD) — two copies in one process abort at exit — and a slab step over
    the communicator (world 1: the exchange lists are empty, the all-reduces real) must run and exit cleanly."""
    pr = children.run([sys.executable, os.path.join(os.path.dirname(HERE), "scripts", "rccl_with_torch.py")], limit=300)
    after = [l for l in pr.output.splitlines() if l.startswith("rccl mapped after:")]
    assert after and after[0].count("librccl") == 1, pr.output[-2000:]
    assert " rc 1 " in after[0] and "closed" in pr.output


def test_bench_single_gpu_line_keeps_the_contract(tmp_path):
    """`python bench.py --full` (N = 1) on a small stand-in (64^3 cavity, 64^3 coil for the strong block, a 32^3 CPU sample): ONE JSON line with the
    driver's keys, the roofline and cpu_baseline objects, and r05's additions — the identity / Chebyshev lines beside the Jacobi headline
     and the box calibration; --dump-outputs writes the last timed step's fields whole (they fit the budget at 64^3)."""
    dump = tmp_path / "out"
    d = _bench_line("--res", "64", "--steps", "2", "--warmup", "1", "--full", "--strong-res", "64", "--cpu-sample-res", "32", "--dump-outputs", str(dump),
                    limit=600)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is False and d["vs_baseline"] is None
    assert d["dtype"] == "f64" and d["data"] == "synthetic" and d["unit"] == "ms/step" and d["value"] == d["ms_per_step"] > 0
    assert "jacobi-PCG" in d["config"]["workload"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and "traffic" in r
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["value"] > 0 and c["cores"] >= 1 and "sample" in c and c["unit"].startswith("ms/step")
    o = d["other_preconditioners"]
    assert set(o) == {"identity", "chebyshev4", "chebyshev4_fp64", "chebyshev10"}
    assert o["chebyshev10"]["cg_iterations"] < o["chebyshev4"]["cg_iterations"]
    assert o["chebyshev4_fp64"]["inner_vectors"] == "fp64" and o["chebyshev4"]["inner_vectors"] in ("fp32", "fp64")   # (fp32 where its kernels run: DESIGN.md)
    assert abs(o["chebyshev4"]["cg_iterations"] - o["chebyshev4_fp64"]["cg_iterations"]) <= max(2, 0.05 * o["chebyshev4_fp64"]["cg_iterations"])
    for v in o.values():
        assert v["result"] == 1 and v["ms_per_step"] > 0 and v["cg_iterations"] > 0
    assert o["chebyshev4"]["cg_iterations"] < d["cg_iterations"]      # the polynomial cuts the count
    assert d["box"]["d2d_copy_GBps"] > 500.0
    assert d["strong_512"]["n_gpus"] == 1 and d["strong_512"]["result"] == 1
    files = {f: np.load(dump / f) for f in os.listdir(dump)}
    shapes = abi.grid_shapes(64, 64, 64)
    assert set(files) == {n + a + ".npy" for n in ("vel", "valid") for a in "XYZ"} | {"dimData.npy", "solve.npy"}
    for a in "XYZ":
        for n in ("vel", "valid"):
            v = files[n + a + ".npy"]
            assert v.dtype == np.float32 and v.size == int(np.prod(shapes["face" + a])) and np.isfinite(v).all()
    assert files["dimData.npy"].dtype == np.float64 and files["dimData.npy"].size == 27
    assert list(files["solve.npy"][[0, 2]]) == [d["result"], d["cg_iterations"]]
    assert sum(os.path.getsize(dump / f) for f in files) <= 64 * 1000 * 1000


def test_bench_plain_line_is_the_headline_alone(tmp_path):
    """`python bench.py` without --full: the headline keys and the timed step's outputs, none of the blocks that take runs of their own."""
    dump = tmp_path / "out"
    d = _bench_line("--res", "64", "--steps", "2", "--warmup", "1", "--dump-outputs", str(dump), limit=300)
    assert d["metric"] == "Stokes-solve wall ms/step (assembly+PCG) on 256^3 grid; CG iters/sec"
    assert d["unit"] == "ms/step" and d["higher_is_better"] is False and d["dtype"] == "f64" and d["value"] == d["ms_per_step"] > 0
    assert d["steps"] == 2 and d["warmup"] == 1 and d["result"] == 1 and d["cg_iterations"] > 0
    for k in ("roofline", "box", "pcie_inclusive_ms", "other_preconditioners", "strong_512", "cpu_baseline"):
        assert k not in d, k
    solve = np.load(dump / "solve.npy")
    assert list(solve[[0, 2]]) == [d["result"], d["cg_iterations"]]
    assert {"vel" + a + ".npy" for a in "XYZ"} <= set(os.listdir(dump))


def test_bench_dump_outputs_sample_within_the_budget(tmp_path):
    """bench.dump_outputs on fields larger than the budget: every file within it, the same sampled entries on every call, and every sampled
    entry one of the whole field's."""
    import bench
    import polystokes_amd
    from polystokes_amd import scenes
    sc, p = scenes.cavity(24, tile=12, pad=2)
    s = polystokes_amd.Solver(0)
    s.upload(sc, p)
    assert s.step_device() == abi.SUCCESS
    budget = 64 << 10
    for tag, b in (("a", budget), ("b", budget), ("whole", bench.DUMP_BUDGET_BYTES)):
        bench.dump_outputs(s, str(tmp_path / tag), budget=b)
    s.close()
    names = sorted(os.listdir(tmp_path / "whole"))
    assert sorted(os.listdir(tmp_path / "a")) == names
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) <= budget
    for f in names:
        a, b, whole = (np.load(tmp_path / t / f) for t in ("a", "b", "whole"))
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
        if f.startswith(("vel", "valid")):
            assert a.size < whole.size and np.isin(a, whole).all()
        else:
            assert np.array_equal(a, whole)

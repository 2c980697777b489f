"""The regions of the PCG vector kernels' shared bodies (ps_kernels_cg.hpp: cgInit, cgUpdateR, cgUpdateXp, k_uinv_pp), pinned for every
element type: the 16-byte loop and the scalar tail from W * nv on (W = 2 doubles or 4 floats per access).  Whether the other suites reach the
tail is an accident of their scenes' sizes; the scenes here are chosen for nSystem % 4 (the oracle's dimData[21], computed on the CPU and
hard-coded below), and every test asserts the residue it relies on first.

NOT covered: the third region, the all-scalar form a kernel takes when a base pointer is not 16-byte aligned.  No caller can produce such a
pointer today: the vectors are device allocations, and a rank's kernels run on x + ownLo with ownLo = 0 — the owned lattice blocks come first
in every rank's numbering ("ownedRange", asserted in the rank test below).  An odd owned count on a rank changes n, not the base: the
rank test walks the one-element tail through Dist's launch sites, no more."""
import pytest

from polystokes_amd import _abi as abi
from polystokes_amd import scenes

import children
import test_gpu_iterates as iterates
import test_gpu_mixed_precision as mixed
from test_gpu_mixed_precision import gpu  # noqa: F401  (the module's solver fixture)

on_gpu = pytest.mark.gpu

# scene (test_gpu_iterates.SCENES) -> (nSystem, nSystem % 4).  tail1-3: scenes.blob(20, 18, 22, seed = 4, 1, 2, tile=8), a viscosity field (the
# fp64 stress diagonal); tail1c: scenes.coil(30, tile=8), the coded one
SIZES = {"tail1": (9169, 1), "tail2": (8806, 2), "tail3": (8579, 3), "tail1c": (42329, 1)}
PRECONDS = ("identity", "jacobi", "cheb4", "cheb32")


def oracle_size(sc, p):
    from oracle import ps_oracle
    o = ps_oracle.Oracle()
    o.run(sc, p, solve=False)
    return int(o.stats.dimData[21])


_checked = {}


def residue(scene):
    """nSystem % 4 of a scene of SIZES, asserted against the oracle (once per scene)"""
    if scene not in _checked:
        n = oracle_size(*iterates.SCENES[scene]())
        assert (n, n % 4) == SIZES[scene], (scene, n)
        _checked[scene] = n % 4
    return _checked[scene]


def test_the_scenes_cover_every_residue():   # (on the CPU: the oracle alone)
    assert {residue(s) for s in SIZES} == {1, 2, 3}


# ---- 1. single domain: x_25 and x_50 against the fp64 reference -------------------------------------------------------------------------
@on_gpu
@pytest.mark.parametrize("pre", PRECONDS)
@pytest.mark.parametrize("scene", list(SIZES))
def test_iterates_on_odd_sizes_five_kernel_step(scene, pre):
    """the step the size decides (these systems are far below the four-kernel step's 1.2 M rows): k_cg_update_r, k_cg_update_xp / _xp_z.
    Measured max |dx| / max |x| on an MI355X (largest of x_25, x_50): tail1-3 identity and Chebyshev-4 5e-16, Jacobi 4.6e-14 .. 1.7e-13, fp32
    polynomial 2.1e-12 .. 3.7e-12; tail1c fp64 steps 6.0e-15 .. 9.4e-15, fp32 polynomial 4.7e-9."""
    assert residue(scene) == SIZES[scene][1]
    out = iterates.run_case(scene, pre, batches=(1, 2))
    assert out["fused"] == 0, out
    print(scene, pre, out["drift"])
    iterates.check(out, pre)


@on_gpu
@pytest.mark.parametrize("scene", list(SIZES))
def test_iterates_on_odd_sizes_four_kernel_step(scene):
    """PS_FUSED_R=1 in a child process (the switch is read once per process): k_uinv_pp, k_cg_update_xp_u / _xp_z_u.
    Measured (as above): tail1-3 fp64 steps 4.1e-16 .. 1.1e-13, fp32 polynomial 2.5e-12 .. 3.3e-12; tail1c 5.9e-15 .. 8.6e-15 and 4.7e-9."""
    assert residue(scene) == SIZES[scene][1]
    res = iterates.run_child({"PS_FUSED_R": "1"}, [[scene, pre] for pre in PRECONDS])
    assert [r["case"][1] for r in res] == list(PRECONDS)
    for r in res:
        assert r["fused"] == 1, r
        print(scene, r["case"][1], r["drift"])
        iterates.check(r, r["case"][1])


# ---- 2. mixed precision: four floats per access ------------------------------------------------------------------------------------------
@on_gpu
@pytest.mark.parametrize("pre", list(mixed.PRECONDS))
@pytest.mark.parametrize("scene", ["tail1", "tail3"])
def test_mixed_solve_on_odd_sizes(gpu, scene, pre):  # noqa: F811
    assert residue(scene) in (1, 3) and residue("tail1") != residue("tail3")
    mixed.mixed_solve_meets_the_rule_and_the_caps(gpu, scene, pre, 1e-6, make=iterates.SCENES[scene])


# ---- 3. two in-process z-slab ranks: an odd and an even number of owned DOFs on the lower rank (its n in Dist's launches) -----------------------
# at most six small candidates, walked in this order (32 or 36 layers: one cut at z = 16)
RANK_CANDIDATES = {
    "blob36_0": lambda: scenes.blob(20, 18, 36, seed=0, tile=8),
    "blob36_1": lambda: scenes.blob(20, 18, 36, seed=1, tile=8),
    "blob36_2": lambda: scenes.blob(20, 18, 36, seed=2, tile=8),
    "blob36_3": lambda: scenes.blob(20, 18, 36, seed=3, tile=8),
    "coil32": lambda: scenes.coil(32, tile=8),
    "spheres32": lambda: scenes.spheres(32, tile=8),
}


def ranks_child():
    """(in the child, PS_FUSED_R=1) the first candidate whose lower rank owns an odd number of DOFs and the first where it is even, each solved
    with Jacobi (the four-kernel step across the cut) and with the polynomial (five kernels, z a vector): test_gpu_multirank's assertions"""
    import polystokes_amd
    from test_gpu_multirank import slabs_match_single_domain
    picks, owned = {}, {}
    single, grp = polystokes_amd.Solver(0), polystokes_amd.Group(2)
    for name, make in RANK_CANDIDATES.items():
        for pre in (abi.PRE_DIAGONAL, abi.PRE_CHEBYSHEV):
            sc, p = make()
            p.preconditioner = pre
            slabs_match_single_domain(single, grp, sc, p, (name, pre))
            lower = int(grp.ranks[0].dist_stats()["owned_dofs"])
            owned[name] = lower
            for r in grp.ranks:     # every rank's owned range starts at DOF 0 of its own numbering: its vectors' bases are the allocations'
                lo, hi = (int(v) for v in r.array("ownedRange"))
                assert lo == 0 and hi == int(r.dist_stats()["owned_dofs"]), (name, lo, hi)
            if lower % 2 in picks:
                break                                   # this parity has its scene already
            assert int(grp.ranks[0].array("fusedStep")[0]) == (1 if pre == abi.PRE_DIAGONAL else 0), (name, pre)
            if pre == abi.PRE_CHEBYSHEV:
                picks[lower % 2] = name
        if len(picks) == 2:
            break
    grp.close()
    single.close()
    return {"odd": picks.get(1), "even": picks.get(0), "owned": owned}


_CHILD = (
    "import test_gpu_vector_tails as t\n"
    "print('RESULT ' + json.dumps(t.ranks_child()))\n"
)


@on_gpu
def test_two_ranks_with_an_odd_and_an_even_cut():
    """Measured on an MI355X: blob36_0's lower rank owns 2552 DOFs (even), blob36_1's 2501 (odd) — the walk ends after two candidates.
    Both ranks' ownedRange starts at 0: the odd count is an odd n (a one-element scalar tail in k_cg_update_r / _xp / _xp_u / _xp_z on a rank),
    not an unaligned base."""
    out = children.run_python(_CHILD, limit=600, env={"PS_FUSED_R": "1"}).result()
    print(out)
    assert out["odd"] is not None and out["even"] is not None, out

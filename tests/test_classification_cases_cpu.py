"""The crafted-weight case table (classification_cases.py) reaches what it is meant to reach: asserted from the CPU oracle alone, through its
fix counters (ps_oracle.hpp: fixCounters, componentSizes).  These are conditions on the cases, not measurements of the library: if one fails,
the case table has lost its point and the GPU tests built on it (test_gpu_classification.py) check less than they claim."""
import numpy as np
import pytest

from polystokes_amd import _abi as abi

import classification_cases as cc


@pytest.fixture(scope="module")
def runs(oracle_mod):
    """name -> (scene, params, oracle run once: with its solve on the cases whose regions feed one)"""
    out = {}
    for name in cc.CASES:
        sc, p = cc.build(name)
        o = oracle_mod.Oracle()
        o.run(sc, p, solve=name in cc.FEED_CASES)
        out[name] = (sc, p, o, o.fix_counters())
    return out


def test_the_table_covers_the_parameter_space(runs):
    ps = [(sc, p) for sc, p, _, _ in runs.values()]
    tiled = [(sc, p) for sc, p in ps if p.doTile]
    assert {3, 4, 23, 24} <= {p.tileSize for _, p in tiled}          # both sides of B >= 4 and of the LDS limit B <= 23
    assert {0, 1, 2} <= {p.tilePadding for _, p in tiled}
    assert {0, 1} == {p.doTile for _, p in ps}
    assert {abi.ORDER_LINEAR, abi.ORDER_VOXEL_TILES} == {p.indexOrder for _, p in ps}
    assert any(all(n % p.tileSize for n in (sc.nx, sc.ny, sc.nz)) for sc, p in tiled)
    assert all(p.activeLiquidBoundaryLayerSize == 1 for _, p in ps)
    assert max(sc.nx * sc.ny * sc.nz for sc, _ in ps) == np.prod(cc.LARGEST_GRID)
    for sc, _ in ps:
        for w in sc.weights:
            assert np.array_equal(w * 8, np.round(w * 8))
        assert all(np.ptp(v) > 0 for v in sc.vel)
    assert set(cc.FEED_CASES) <= set(cc.CASES) and set(cc.SERPENTINES) <= set(cc.CASES)


def test_counters_are_consistent(runs):
    for name, (sc, p, o, c) in runs.items():
        assert c["sweeps"] >= 1 and c["fixes"] >= c["fixes_by_demoted"] >= 0, name
        assert (c["sweeps"] == 1) == (c["fixes"] == 0), name          # the last sweep is the idle one
        assert c["regions_before"] == len(o.array("componentSizeCounters")), name
        assert c["regions_after"] == o.nRegions <= c["regions_before"] - c["regions_emptied"], name


def test_sweeps_and_fixes_by_demoted_cells(runs):
    assert sum(c["sweeps"] >= 3 for _, _, _, c in runs.values()) >= 3
    acting = [(p.indexOrder, p.doTile) for _, p, _, c in runs.values() if c["fixes_by_demoted"] >= 100]
    assert len(acting) >= 3
    assert {abi.ORDER_LINEAR, abi.ORDER_VOXEL_TILES} <= {o for o, _ in acting}
    assert any(t for _, t in acting)
    # a second sweep that applies fixes (three sweeps: two that apply, one idle)
    assert any(c["sweeps"] >= 3 and c["fixes"] > 0 for _, _, _, c in runs.values())


def test_regions_emptied_and_removed(runs):
    assert any(2 * c["regions_emptied"] > c["regions_before"] for _, _, _, c in runs.values())
    gone = [(o, c) for _, _, o, c in runs.values() if c["regions_before"] > 0 and c["regions_after"] == 0]
    assert gone
    for o, c in gone:
        assert o.stats.dimData[24] == 0 and o.stats.dimData[11] == 0          # no region, no reduced velocity DOF: active DOFs only
        assert o.nA > 0 and o.nP > 0
        assert not (o.array("centerLabels") == cc.PS_REDUCED).any()
    # regionCount going to 0 and back is what the state test steps through
    assert runs["walls_12x10x14_linear"][3]["regions_after"] == 0 and runs["maze_t8p1"][3]["regions_after"] > 0


def test_overlapping_and_unfilled_boxes(runs):
    overlapping = {}
    unfilled = {}
    for name, (sc, p, o, c) in runs.items():
        box, cells = cc.region_boxes(o)
        R = len(cells)
        assert (cells > 0).all(), name
        pairs = [(a, b) for a in range(R) for b in range(a + 1, R) if cc.boxes_overlap(box[a], box[b])]
        if pairs:
            T = p.tileSize
            same_tile = any((box[a, :3] // T == box[b, :3] // T).all() for a, b in pairs)
            overlapping[name] = (bool(p.doTile), same_tile)
        unfilled[name] = int((cells < np.prod(box[:, 3:] - box[:, :3] + 1, axis=1)).sum())
    assert len(overlapping) >= 2
    assert any(tile and same for tile, same in overlapping.values())          # tiled, two regions in one tile
    assert any(not tile for tile, _ in overlapping.values())                 # doTile = 0
    assert max(unfilled.values()) >= 5
    for name in cc.FEED_CASES:                                                # every one of them has regions left for the blocks
        assert runs[name][2].nRegions >= 2, name


@pytest.mark.parametrize("name", list(cc.SERPENTINES))
def test_serpentine_components(runs, name):
    n, B, pad, mirrored = cc.SERPENTINES[name]
    sc, p, o, c = runs[name]
    assert (sc.nx, sc.ny, sc.nz) == n and p.tileSize == B and p.tilePadding == pad and p.doTile == 1
    paths = cc.serpentine_paths(n, B, pad, mirrored)
    sizes = o.array("componentSizeCounters")
    assert sorted(sizes) == sorted(len(q) for q in paths)                    # exactly one component per tile, its whole snake
    long_ = [q for q in paths if len(q) >= 4 * B * B + 1]
    full = (n[0] // B) * (n[1] // B) * (n[2] // B)
    assert len(long_) >= max(full, 1)                                        # every full tile's, and at least one
    for q in paths:
        assert q[0] == tuple(np.min(q, axis=0))                               # the smallest traversal index is one end of the path
    if full:
        assert sum(len(q) == (B - pad) ** 3 for q in paths) == full


@pytest.mark.parametrize("name", cc.FEED_CASES)
def test_the_oracles_own_blocks_and_solve_are_sound(runs, name):
    """what test_tile_blocks_match asks of the library's BInv holds for the oracle's own, and its solve succeeds"""
    sc, p, o, c = runs[name]
    R = o.nRegions
    Mr = o.array("reducedMassMatrices").reshape(R, 26, 26)
    K = o.array("reducedViscosityMatrices").reshape(R, 26, 26)
    Bo = o.array("Inv_Mr_plus_2JDtuDJ").reshape(R, 26, 26)
    for r in range(R):
        assert np.abs(Bo[r] @ (Mr[r] / sc.dt + 2 * K[r]) - np.eye(26)).max() < 1e-7, (name, r)
    # the fit of a region's velocity has one solution: a singular system (a region with ACTIVE cells on too few sides; about 1e18 here) leaves
    # the fit, and the reduced right-hand side made from it, to the pivoting of whoever solves it.  fp64 and the 1e-8 asked of that right-hand
    # side leave room for 1e8.
    N = o.array("reducedRegionBestFitSystems").reshape(R, 26, 26)
    for r in range(R):
        assert np.linalg.cond(N[r]) < 1e8, (name, r)
    assert o.result == abi.SUCCESS and o.stats.usedBiCGStab == 0 and o.stats.solveData[1] > 10, name

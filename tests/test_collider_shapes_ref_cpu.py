"""The numpy restatement of ps_place_colliders (collider_shapes_ref.py) on its own, without a GPU: the properties the header promises, and
that the shared cases (collider_shapes_cases.py) tell the rule from its near misses.  test_gpu_collider_shapes.py compares the device with
this restatement byte for byte."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import collider_shapes_cases as cases  # noqa: E402
import collider_shapes_ref as ref  # noqa: E402


def test_a_volume_on_the_world_lattice_is_copied_exactly():
    sc, p, ids, shapes, poses, col, idf, counters = cases.build("lattice")
    sdf = shapes[0][0]
    box = (slice(2, 7), slice(3, 9), slice(6, 14))                   # sample (i, j, k) on cell (6 + i, 3 + j, 2 + k)
    base = sc.collision[box]
    wins = sdf < base                                                # D_k = -sdf against D = -base, strictly
    assert wins.any() and (~wins).any()
    assert np.array_equal(col[box][wins].view(np.uint32), sdf[wins].view(np.uint32))
    assert np.array_equal(col[box][~wins].view(np.uint32), base[~wins].view(np.uint32))
    assert np.array_equal(idf[box], np.where(wins, 0, -1))
    assert counters.sum() == sc.nx * sc.ny * sc.nz and counters[-1] == 0


@pytest.mark.parametrize("case", ["three_negate", "three_no_negate", "count64", "spacings"])
def test_a_second_placement_leaves_values_and_ids(case):
    sc, p, ids, shapes, poses, col, idf, counters = cases.build(case)
    col2, idf2, counters2 = ref.place(col, idf, shapes, poses, sc.orig, sc.dx, p.negateCollision)
    assert np.array_equal(col2.view(np.uint32), col.view(np.uint32)) and np.array_equal(idf2, idf)
    assert counters2.sum() == counters.sum()


@pytest.mark.parametrize("case", ["three_negate", "three_orig", "spacings"])
def test_cells_beyond_the_reach_are_untouched(case):
    sc, p, ids, shapes, poses, col, idf, counters = cases.build(case)
    k, j, i = np.indices(sc.collision.shape)
    r = np.stack([sc.orig[0] + (i + 0.5) * sc.dx, sc.orig[1] + (j + 0.5) * sc.dx, sc.orig[2] + (k + 0.5) * sc.dx], axis=-1)
    near = np.zeros(sc.collision.shape, bool)       # within the reach of some volume, by the matrix form of the transform and a margin
    far = np.ones(sc.collision.shape, bool)
    for (sdf, h, o), P in zip(shapes, poses):
        R, t = P[:9].reshape(3, 3), P[9:]
        s = ((r - t) @ R - o) / h - 0.5
        n = np.array(sdf.shape[::-1], np.float64)
        E = ref.REACH * sc.dx / h
        over = np.maximum(np.maximum(-s, s - (n - 1)), 0.0).max(axis=-1)       # samples beyond the box, largest axis
        near |= over < E - 1e-9
        far &= over > E + 1e-9
    assert far.any() and near.any()
    assert np.array_equal(col[far].view(np.uint32), sc.collision[far].view(np.uint32))
    want_ids = np.full(idf.shape, -1, np.int32) if ids is None else ids
    assert np.array_equal(idf[far], want_ids[far])
    changed = col.view(np.uint32) != sc.collision.view(np.uint32)
    assert changed[near].any() and not changed[far].any()
    beyond_box = np.ones(sc.collision.shape, bool)                  # ... and some changed cell lies outside every box: the continuation is used
    for (sdf, h, o), P in zip(shapes, poses):
        s = ((r - P[9:]) @ P[:9].reshape(3, 3) - o) / h - 0.5
        beyond_box &= ((s < -0.01) | (s > np.array(sdf.shape[::-1]) - 0.99)).any(axis=-1)
    assert (changed & beyond_box).any()


def test_ties_go_to_the_cell_then_to_the_lower_collider():
    # identical pairs: the upper of each never wins a cell
    sc, p, ids, shapes, poses, col, idf, counters = cases.build("count64")
    assert counters[10] > 0 and counters[40] > 0 and counters[11] == 0 and counters[41] == 0
    assert not np.isin(idf[col.view(np.uint32) != sc.collision.view(np.uint32)], (11, 41)).any()
    # a cell that already holds exactly what the volume gives keeps its id
    sc, p, ids, shapes, poses, col, idf, counters = cases.build("lattice")
    base = sc.collision.copy()
    base[2:7, 3:9, 6:14] = shapes[0][0]
    col2, idf2, counters2 = ref.place(base, None, shapes, poses, sc.orig, sc.dx, 1)
    assert (idf2[2:7, 3:9, 6:14] == -1).all()
    assert np.array_equal(col2[2:7, 3:9, 6:14].view(np.uint32), shapes[0][0].view(np.uint32))


def test_a_rotated_sphere_reproduces_the_analytic_sphere():
    """radius 0.2 in a 24^3 volume at h = 1/40, placed into a 32^3 grid at dx = 1/32 by a random rotation about (0.5, 0.5, 0.5): within
    2 dx of the surface the trilinear resampling stays within 0.1 dx of the distance (0.035 dx on the prototype)"""
    n, dx = 32, 1.0 / 32.0
    rng = np.random.RandomState(21)
    shape = cases.sphere_volume(0.2, 24, 1.0 / 40.0)
    centre = np.array([0.5, 0.5, 0.5])
    P = cases.pose(shape, cases.rotation(rng), centre).reshape(1, 12)
    base = np.full((n, n, n), 10.0, np.float32)
    col, idf, counters = ref.place(base, None, [shape], P, (0.0, 0.0, 0.0), dx, 1)
    q = (np.arange(n) + 0.5) * dx
    z, y, x = np.meshgrid(q, q, q, indexing="ij")
    exact = np.sqrt((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2) - 0.2
    band = np.abs(exact) < 2.0 * dx
    assert band.sum() > 1000 and (idf[band] == 0).all()
    err = np.abs(col[band].astype(np.float64) - exact[band]).max() / dx
    print("largest error within 2 dx of the surface: %.4f dx" % err)
    assert err <= 0.1


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_the_cases_tell_the_rule_from_its_near_misses(mutant):
    caught = []
    for case in sorted(cases.CASES):
        sc, p, ids, shapes, poses, col, idf, counters = cases.build(case)
        c2, i2, n2 = ref.place(sc.collision, ids, shapes, poses, sc.orig, sc.dx, p.negateCollision, mutant=mutant)
        if not (np.array_equal(c2.view(np.uint32), col.view(np.uint32)) and np.array_equal(i2, idf) and np.array_equal(n2, counters)):
            caught.append(case)
    print(mutant, "changes", caught)
    assert caught, mutant


def test_the_cases_cover_what_they_claim():
    for case in sorted(cases.CASES):
        sc, p, ids, shapes, poses, col, idf, counters = cases.build(case)
        assert counters.sum() == sc.nx * sc.ny * sc.nz, case
        print(case, counters.tolist())
    n = cases.build("count64")[7]
    assert (n[5:64:8] == 0).all() and (n[:64] > 0).sum() > 20                    # the volumes off the grid win nothing, many others do
    n = cases.build("deep_base")[7]
    assert n.tolist() == [0, 0, 0, 20 * 12 * 9, 0]
    n = cases.build("larger")[7]
    assert n[0] > 0.3 * 20 * 12 * 9
    for case in ("three_negate", "three_no_negate", "three_orig", "spacings"):
        assert (cases.build(case)[7][:-2] > 0).all(), case

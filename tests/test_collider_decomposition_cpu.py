"""Collider placement and painting on slab and brick ranks, without a GPU: what test_gpu_collider_decomposition.py relies on, shown on the
numpy restatements alone (collider_shapes_ref.py, collider_motions_ref.py through collider_decomposition_cases.rank_expected).

A rank's result is the rule on its own grid.  It equals the global result cut to the rank's grid byte for byte, with one exception that
the paint's rule itself makes: a face of axis a on the outermost plane of a side with a neighbour has one cell on the rank and two in the
whole grid."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import collider_decomposition_cases as cases  # noqa: E402

from polystokes_amd import partition  # noqa: E402

BOX = sorted(cases.CASES)
expected = cases.expected


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("case", BOX)
def test_rank_result_equals_the_global_result_cut_to_the_rank(case):
    c = cases.build(case)
    differing = 0
    for g, (col, idf, placed, grids, faces) in zip(c.geo, expected(case)):
        assert np.array_equal(bits(col), bits(g.cut(c.col))), (case, g.rank, "collision")
        assert np.array_equal(idf, g.cut(c.idf)), (case, g.rank, "ids")
        for a in range(3):
            want, outer = g.cut(c.grids[a], a), g.outer_planes(a)
            diff = bits(grids[a]) != bits(want)
            assert not diff[~outer].any(), (case, g.rank, a, np.argwhere(diff & ~outer)[:4].tolist())
            if outer.any():                                        # the exception is no dead code: some faces of every such plane set differ
                print(case, "rank", g.rank, "axis", a, "outer-plane faces", int(outer.sum()), "differing", int(diff[outer].sum()))
                assert diff[outer].any(), (case, g.rank, a)
                differing += int(diff[outer].sum())
            else:
                assert not diff.any()
    assert differing > 0


def face_colliders(col, idf, a, negate, count):
    """the collider every face of axis a is painted for (-1: left alone), by the restatement's own choice of the cell"""
    chosen, _ = cases.motions_ref.chosen_cells(col, a, negate)
    k = idf[chosen]
    return np.where((k >= 0) & (k < count), k, -1)


@pytest.mark.parametrize("case", BOX)
def test_counters_are_those_of_the_ranks_grid_and_add_up_over_owned_samples(case):
    c = cases.build(case)
    count, negate = len(c.shapes), c.params.negateCollision
    winner_global = np.where(bits(c.col) != bits(c.scene.collision), c.idf, -1)          # (a won cell changes its value)
    assert np.array_equal(np.bincount(winner_global[winner_global >= 0], minlength=count), c.placed[:count])
    faces_global = [face_colliders(c.col, c.idf, a, negate, count) for a in range(3)]
    assert np.array_equal(sum(np.bincount(f[f >= 0], minlength=count) for f in faces_global), c.faces[:count])
    cells_sum, faces_sum = np.zeros(count, np.int64), np.zeros(count, np.int64)
    for g, (col, idf, placed, grids, faces) in zip(c.geo, expected(case)):
        # per rank: the counters of the rank's own grid, halo blocks included
        winner = np.where(bits(col) != bits(g.cut(c.scene.collision)), idf, -1)
        assert np.array_equal(np.bincount(winner[winner >= 0], minlength=count), placed[:count]), (case, g.rank)
        assert placed[count] == int((winner < 0).sum()) and placed.sum() == g.n[0] * g.n[1] * g.n[2]
        own = g.owned_cells()
        assert np.array_equal(winner[own], g.cut(winner_global)[own])
        cells_sum += np.bincount(winner[own & (winner >= 0)], minlength=count)
        per_axis = [face_colliders(col, idf, a, negate, count) for a in range(3)]
        assert np.array_equal(sum(np.bincount(f[f >= 0], minlength=count) for f in per_axis), faces[:count]), (case, g.rank)
        assert faces.sum() == sum(f.size for f in per_axis)
        for a in range(3):
            f = g.owned_faces(a)
            assert not (f & g.outer_planes(a)).any()
            assert np.array_equal(per_axis[a][f], g.cut(faces_global[a], a)[f]), (case, g.rank, a)
            faces_sum += np.bincount(per_axis[a][f & (per_axis[a] >= 0)], minlength=count)
    # every cell and every face has exactly one owner: the owned sums are the global counters
    assert np.array_equal(cells_sum, c.placed[:count]), (cells_sum.tolist(), c.placed.tolist())
    assert np.array_equal(faces_sum, c.faces[:count]), (faces_sum.tolist(), c.faces.tolist())


def shifted(c, g, mutant):
    """the orig a wrong helper would hand rank g"""
    o, dx = np.array(c.scene.orig, np.float64), c.scene.dx
    if mutant == "not_shifted":
        return tuple(o)
    if mutant == "owned_lower_bound":                              # g0 instead of g0 - lo_halo
        return tuple(o + np.array([g.origin[a] + g.lo[a] for a in range(3)], np.float64) * dx)
    assert mutant == "wrong_axis"                                  # x and z exchanged
    return tuple(o + np.array(g.origin[::-1], np.float64) * dx)


MUTANTS = ("not_shifted", "owned_lower_bound", "wrong_axis")


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_case_tells_the_helper_from_its_near_misses(mutant):
    applies = 0
    for case in BOX:
        c = cases.build(case)
        changed = []
        for g, want in zip(c.geo, expected(case)):
            o = shifted(c, g, mutant)
            if o == tuple(cases.local(case, c.parts[g.rank])[0].orig):
                continue                                           # the mutant hands this rank the right orig
            got = cases.rank_expected(case, c.parts[g.rank], orig=o)
            same = (np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
                    and all(np.array_equal(bits(a), bits(b)) for a, b in zip(got[3], want[3])))
            if not same:
                changed.append(g.rank)
        affected = [g.rank for g in c.geo if any(g.origin)] if mutant != "wrong_axis" else [g.rank for g in c.geo if g.origin[0] != g.origin[2]]
        print(mutant, case, "ranks with another orig", affected, "changed", changed)
        if affected:
            applies += 1
            assert changed, (mutant, case)
    assert applies == len(BOX)                                     # every box case has a rank with a non-zero origin on an affected axis


def test_the_helper_gives_every_rank_the_orig_of_its_block():
    for case in BOX:
        c = cases.build(case)
        for part, g in zip(c.parts, c.geo):
            sc = cases.local(case, part)[0]
            want = tuple(float(c.scene.orig[m]) + float(g.origin[m]) * float(c.scene.dx) for m in range(3))
            assert tuple(sc.orig) == want and all(isinstance(v, float) for v in sc.orig), (case, g.rank)
            assert all(sc.orig[m] == c.scene.orig[m] for m in range(3) if g.origin[m] == 0)          # origin 0 keeps the given value
    # without a scene orig: zeros shifted by the origin; the arrays are the cuts they were
    c = cases.build("box_z3")
    import copy
    plain = copy.copy(c.scene)
    del plain.orig
    for part, g in zip(c.parts, c.geo):
        sc = partition.local_scene(plain, part)
        assert tuple(sc.orig) == (0.0, 0.0, g.origin[2] * c.scene.dx)
        assert np.array_equal(sc.collision, g.cut(c.scene.collision)) and np.array_equal(sc.collisionvel[2], g.cut(c.scene.collisionvel[2], 2))
    # an axis that is not cut is one range of any length, shorter than a halo block too (ny = 12 and nz = 20 of the boxes); a cut one is not
    assert partition.slab_ranges(12, 1, 16) == [(0, 12)] and partition.slab_ranges(20, 1, 16) == [(0, 20)]
    assert partition.slab_ranges(48, 1, 16) == [(0, 48)] and partition.slab_ranges(48, 2, 16) == [(0, 32), (32, 48)]
    with pytest.raises(ValueError):
        partition.slab_ranges(20, 2, 16)
    b = partition.make_brick((48, 12, 20), (2, 1, 1), 1, 8)
    assert b.origin == [16, 0, 0] and b.n_local == [32, 12, 20] and b.hasLower == [1, 0, 0] and b.hasUpper == [0, 0, 0]


@pytest.mark.parametrize("case", BOX)
def test_the_cases_cover_what_they_claim(case):
    c = cases.build(case)
    count = len(c.shapes)
    won = bits(c.col) != bits(c.scene.collision)
    winner = np.where(won, c.idf, -1)
    n = (c.scene.nx, c.scene.ny, c.scene.nz)
    # a volume that wins cells on both sides of every cut
    for a in range(3):
        for cut in c.cuts[a]:
            below, above = [slice(None)] * 3, [slice(None)] * 3
            below[2 - a], above[2 - a] = slice(0, cut), slice(cut, n[a])
            both = set(np.unique(winner[tuple(below)])) & set(np.unique(winner[tuple(above)])) - {-1}
            print(case, "axis", a, "cut", cut, "volumes on both sides", sorted(both))
            assert both, (case, a, cut)
            near = [slice(None)] * 3                               # ... and right at the cut: in the two layers that touch it
            near[2 - a] = slice(cut - 1, cut + 1)
            assert (winner[tuple(near)] >= 0).any()
    # some rank wins cells in a halo block from a volume that wins none of its owned cells
    halo_only = []
    for g, (col, idf, placed, grids, faces) in zip(c.geo, expected(case)):
        own = g.owned_cells()
        w = np.where(bits(col) != bits(g.cut(c.scene.collision)), idf, -1)
        only = set(np.unique(w[~own])) - set(np.unique(w[own])) - {-1}
        if only:
            halo_only.append((g.rank, sorted(only)))
        # the painted-face share per collider is above zero on every rank that the collider reaches
        reached = np.unique(w[w >= 0])
        assert (faces[reached] > 0).all(), (case, g.rank, faces.tolist())
        assert placed[-1] == 0
    print(case, "halo-only winners", halo_only)
    assert halo_only, case
    # one volume wholly off the grid; an id outside the count; no more than half of all cells left alone
    assert c.placed[3 if count == 5 else 5] == 0 and (c.placed[:count] > 0).sum() >= min(count, 4) - 1
    if c.ids is not None:
        assert (c.ids >= count).any() and c.faces[count] > 0
    print(case, "cells", c.placed.tolist(), "faces", c.faces.tolist())
    assert 2 * int(c.placed[count]) <= won.size, (case, int(c.placed[count]), won.size)
    if case == "box_ties":                                         # neighbours that tie, on the planes of the cuts too
        D = -c.col.astype(np.float64)
        for a in range(3):
            for cut in c.cuts[a]:
                lo, up = [slice(None)] * 3, [slice(None)] * 3
                lo[2 - a], up[2 - a] = cut - 1, cut
                base = -c.scene.collision.astype(np.float64)
                assert (base[tuple(lo)] == base[tuple(up)]).mean() > 0.1 and (D[tuple(lo)] == D[tuple(up)]).any()


def test_the_stepping_scene_puts_its_volumes_where_it_says():
    sc, p, shapes, poses, motions = cases.step_scene()
    assert sc.nx == sc.ny == sc.nz == 64 and p.tileSize == 8
    sc2, p2, placed, faces = cases.placed_step_scene()
    print("stepping scene: cells", placed.tolist(), "faces", faces.tolist())
    assert (placed[:3] > 50).all() and (faces[:3] > 0).all()
    won = bits(sc2.collision) != bits(sc.collision)
    k, j, i = np.nonzero(won)
    assert (i < 32).any() and (i >= 32).any() and (k < 32).any() and (k >= 32).any()    # across the x cut and the z cut
    # What run (b) of the GPU test gives the solve and what run (c) does differ, and on the outer planes alone: the ranks' own restated
    # paint against the cut of the global one.  "The solve does not read that plane" rests on this being more than nothing.
    n = (sc.nx, sc.ny, sc.nz)
    for case, (dims, world) in sorted(cases.STEP_CASES.items()):
        assert [q for q in cases.cut_axes(n, dims, world) if q]
        differing = 0
        for part in cases.make_parts(n, dims, world):
            g = cases.Geometry(part, n)
            loc = partition.local_scene(sc, part) if dims is None else partition.local_scene_brick(sc, part)
            col, idf, _ = cases.shapes_ref.place(loc.collision, None, shapes, poses, loc.orig, loc.dx, 1)
            grids, _ = cases.motions_ref.paint(col, idf, motions, loc.orig, loc.dx, 1, loc.collisionvel)
            assert np.array_equal(bits(col), bits(g.cut(sc2.collision))), (case, g.rank)
            for a in range(3):
                diff, outer = bits(grids[a]) != bits(g.cut(sc2.collisionvel[a], a)), g.outer_planes(a)
                assert not diff[~outer].any(), (case, g.rank, a)
                differing += int(diff[outer].sum())
                print(case, "rank", g.rank, "axis", a, "outer-plane faces", int(outer.sum()), "differing", int(diff[outer].sum()))
        assert differing > 0, case

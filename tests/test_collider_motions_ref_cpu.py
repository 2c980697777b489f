"""The numpy restatement of ps_paint_collider_velocities (collider_motions_ref.py) checked on its own, without a GPU: exact values where the
rule has them, the tie / NaN / border rules on crafted SDFs, the counters, and near misses of the rule that the shared cases must catch —
the GPU test compares the device with this restatement byte for byte, so what the restatement cannot tell apart the GPU test cannot either."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import collider_motions_cases as cases  # noqa: E402
import collider_motions_ref as ref  # noqa: E402


def _faces(sc):
    return (sc.nx + 1) * sc.ny * sc.nz + sc.nx * (sc.ny + 1) * sc.nz + sc.nx * sc.ny * (sc.nz + 1)


def test_pure_translation_paints_exactly_v():
    sc, p, ids, tab, grids, counters = cases.build("blob_translation")
    assert not tab[:, 3:].any()
    for a in range(3):
        assert grids[a].dtype == np.float32
        assert np.all(grids[a] == np.float32(tab[0, a]))
    assert counters.tolist() == [_faces(sc), 0, 0]


def test_one_collider_on_the_whole_grid_is_divergence_free():
    """u_a of a rigid motion does not depend on the position along a — the painted component of w x arm holds no arm[a] — so the discrete
    divergence is exactly 0, whatever v, w, o and orig are"""
    sc, p, _, _, _, _ = cases.build("blob_mod3_both")
    tab = cases.table("both", 1, seed=11)
    assert tab[:, 3:6].any()
    grids, counters = ref.paint(sc.collision, None, tab, sc.orig, sc.dx)
    assert counters.tolist() == [_faces(sc), 0, 0]
    assert not ref.divergence(grids, sc.dx).any()
    for a in range(3):                                                  # and it is no constant: the rotation shows
        assert np.unique(grids[a]).size > 1


def test_a_rotation_matches_the_cross_product_written_out():
    sc, p, ids, tab, grids, _ = cases.build("box_rotation")
    ox, oy, oz = sc.orig
    for a, (k, j, i) in ((0, (4, 5, 7)), (1, (2, 12, 3)), (2, (9, 0, 19)), (0, (0, 0, 0))):
        chosen, _ = ref.chosen_cells(sc.collision, a)
        cid = int(ids[chosen[0][k, j, i], chosen[1][k, j, i], chosen[2][k, j, i]])
        if cid >= tab.shape[0]:
            assert grids[a][k, j, i] == sc.collisionvel[a][k, j, i]
            continue
        r = np.array([ox + (i + (0.0 if a == 0 else 0.5)) * sc.dx, oy + (j + (0.0 if a == 1 else 0.5)) * sc.dx, oz + (k + (0.0 if a == 2 else 0.5)) * sc.dx])
        want = tab[cid, 0:3] + np.cross(tab[cid, 3:6], r - tab[cid, 6:9])
        assert abs(float(grids[a][k, j, i]) - want[a]) <= 1e-6 * (1.0 + abs(want[a]))


def _two_cells(dl, du, ids=(0, 1), negate=1):
    """a 1 x 1 x 2 grid: the lower cell's SDF, the upper one's; returns the x-face grid and the counters of a two-collider translation table"""
    col = np.array([[[dl, du]]], np.float32)
    tab = np.zeros((2, 9))
    tab[0, 0], tab[1, 0] = 10.0, 20.0
    g, n = ref.paint(col, np.array([[ids]], np.int32), tab, (0.0, 0.0, 0.0), 1.0, negate)
    return g[0].ravel().tolist(), n.tolist()


def test_tie_nan_and_border_rules():
    # borders take their only cell; the middle face the more solid one (negateCollision = 1: the smaller SDF)
    assert _two_cells(-1.0, 1.0)[0] == [10.0, 10.0, 20.0]
    assert _two_cells(1.0, -1.0)[0] == [10.0, 20.0, 20.0]
    assert _two_cells(0.5, 0.5)[0] == [10.0, 10.0, 20.0]                # a tie: the lower cell
    assert _two_cells(np.nan, -1.0)[0] == [10.0, 10.0, 20.0]            # NaN on either side: the lower cell
    assert _two_cells(-1.0, np.nan)[0] == [10.0, 10.0, 20.0]
    assert _two_cells(-1.0, 1.0, negate=0)[0] == [10.0, 20.0, 20.0]     # negateCollision = 0: the larger SDF is the more solid
    assert _two_cells(1.0, -1.0, negate=0)[0] == [10.0, 10.0, 20.0]
    assert _two_cells(0.0, -0.0)[0] == [10.0, 10.0, 20.0]               # -0 == +0: a tie
    g, n = _two_cells(-1.0, 1.0, ids=(-1, 2))                           # ids outside 0..count-1: left alone (zeros here), slot count
    assert g == [0.0, 0.0, 0.0] and n == [0, 0, 3 + 4 + 4, 0]
    # the y and z faces of that grid: each cell's two faces take the cell (y: 4 faces, z: 4 faces), the x faces as above
    assert _two_cells(-1.0, 1.0)[1] == [2 + 2 + 2, 1 + 2 + 2, 0, 0]


def test_a_non_finite_motion_leaves_its_faces_alone():
    sc, p, ids, tab, grids, counters = cases.build("blob_mod3_both")
    bad = tab.copy()
    bad[1, 4] = np.nan
    g2, n2 = ref.paint(sc.collision, ids, bad, sc.orig, sc.dx, 1, sc.collisionvel)
    assert n2[4] == counters[1] > 0 and n2[1] == 0 and n2[0] == counters[0] and n2[2] == counters[2] and n2[3] == counters[3]
    for a in range(3):
        chosen, _ = ref.chosen_cells(sc.collision, a)
        one = ids[chosen] == 1
        assert np.array_equal(g2[a][one], sc.collisionvel[a][one])
        assert np.array_equal(g2[a][~one], grids[a][~one])


@pytest.mark.parametrize("case", sorted(cases.CASES))
def test_counters_sum_to_the_faces(case):
    sc, p, ids, tab, grids, counters = cases.build(case)
    assert counters.size == tab.shape[0] + 2 and int(counters.sum()) == _faces(sc)
    assert counters[-1] == 0                                            # every table of the cases is finite
    if case in ("box_rotation", "box_count64", "spheres_nearest"):
        assert counters[-2] > 0                                         # ids outside the count occur
        kept = sum(int((grids[a] == sc.collisionvel[a]).sum()) for a in range(3))
        assert kept >= counters[-2]
    if case == "box_count64":
        assert np.all(counters[:64] > 0)


def _differs(case, mutant):
    sc, p, ids, tab, grids, counters = cases.build(case)
    g, n = ref.paint(sc.collision, ids, tab, sc.orig, sc.dx, p.negateCollision, sc.collisionvel, mutant)
    return any(not np.array_equal(g[a].view(np.uint32), grids[a].view(np.uint32)) for a in range(3)) or not np.array_equal(n, counters)


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_mutants_are_caught(mutant):
    caught = [c for c in sorted(cases.CASES) if _differs(c, mutant)]
    print(mutant, "caught by", caught)
    assert caught
    if mutant == "tie_upper":
        assert "box_ties" in caught                                     # the crafted SDF is what tells a tie rule


def test_the_crafted_sdfs_hold_what_they_are_for():
    sc = cases.build("box_ties")[0]
    D = -sc.collision
    assert sum(int((np.diff(D, axis=ax) == 0).sum()) for ax in range(3)) > 100
    assert np.isnan(cases.build("box_nan")[0].collision).sum() == 4
    # the NaN cells decide faces: the rule differs from "NaN to the upper cell" there
    sc, p, ids, tab, grids, _ = cases.build("box_nan")
    flipped = 0
    for a in range(3):
        chosen, other = ref.chosen_cells(sc.collision, a)
        nan_pair = np.isnan(sc.collision[chosen]) | np.isnan(sc.collision[other])
        differs = (chosen[2 - a] != other[2 - a])
        flipped += int((nan_pair & differs).sum())
        assert np.all(chosen[2 - a][nan_pair & differs] < other[2 - a][nan_pair & differs])
    assert flipped >= 12


def test_the_position_along_the_axis_cannot_show():
    """The issue lists "cell-centre instead of grid-line position along a" among the mutants.  Component a of w x arm is
    w[a1] arm[a2] - w[a2] arm[a1]: arm[a] does not occur, so that change alters no painted value on any input.  It is pinned as neutral
    here; the position mutant that can show — grid lines instead of cell centres on the transverse axes — is in MUTANTS."""
    for case in sorted(cases.CASES):
        for mutant in ref.NEUTRAL_MUTANTS:
            assert not _differs(case, mutant), (case, mutant)

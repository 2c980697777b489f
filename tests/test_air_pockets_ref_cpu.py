"""The restatement of the air pockets (air_pockets_ref.py) on cases countable by hand — weights written directly on a 6 x 5 x 4 grid — and two
mutants of it that these cases catch.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import air_pockets_cases as cases  # noqa: E402

U = 1048576          # units of a cell full of air
DX = 0.25


def _air(w, i, j, k, lw=0.0):
    w["lw"][k, j, i] = lw


def split_pair(closed):
    """two air cells side by side in x; the face between them solid (fwF = 0) or open"""
    w = cases.liquid_weights()
    _air(w, 1, 2, 1)
    _air(w, 2, 2, 1)
    if closed:
        w["fwx"][1, 2, 2] = 0.0
    return w


def test_a_solid_face_splits_and_an_open_one_joins():
    r = cases.run_ref(split_pair(True), DX)
    assert r["units"].tolist() == [U, U] and r["cells"].tolist() == [1, 1] and r["open"].tolist() == [0, 0]
    assert r["ids"][1, 2, 1] == 0 and r["ids"][1, 2, 2] == 1 and (r["ids"] >= 0).sum() == 2
    r = cases.run_ref(split_pair(False), DX)
    assert r["units"].tolist() == [2 * U] and r["cells"].tolist() == [2] and r["open"].tolist() == [0]
    assert r["ids"][1, 2, 1] == 0 and r["ids"][1, 2, 2] == 0
    assert r["volume"].tolist() == [(float(2 * U) * (1.0 / 1048576.0)) * (DX * DX * DX)] == [2 * DX ** 3]


def test_a_tied_skin_cell_goes_to_the_first_direction():
    w = cases.liquid_weights()
    _air(w, 1, 2, 1)
    _air(w, 3, 2, 1)
    _air(w, 2, 2, 1, lw=0.75)                      # not core, between the two pockets: both neighbours have lw = 0
    r = cases.run_ref(w, DX)
    assert r["cells"].tolist() == [1, 1]
    assert r["ids"][1, 2, 2] == 0                 # -x comes first
    assert r["units"].tolist() == [U + U // 4, U]
    _air(w, 1, 2, 1, lw=0.25)                      # now the +x neighbour holds less liquid
    r = cases.run_ref(w, DX)
    assert r["ids"][1, 2, 2] == 1
    assert r["units"].tolist() == [3 * U // 4, U + U // 4]
    w["fwx"][1, 2, 3] = 0.0                        # ... but the face towards it is solid
    r = cases.run_ref(w, DX)
    assert r["ids"][1, 2, 2] == 0
    w["fwx"][1, 2, 2] = 0.0                        # both closed: no skin
    r = cases.run_ref(w, DX)
    assert r["ids"][1, 2, 2] == -1 and r["units"].tolist() == [3 * U // 4, U]


def test_half_liquid_is_core_and_five_eighths_is_not():
    w = cases.liquid_weights()
    _air(w, 2, 2, 2, lw=0.5)
    r = cases.run_ref(w, DX)
    assert r["units"].tolist() == [U // 2] and r["cells"].tolist() == [1] and r["ids"][2, 2, 2] == 0
    _air(w, 2, 2, 2, lw=0.625)
    r = cases.run_ref(w, DX)
    assert r["units"].size == 0 and r["cells"].size == 0 and r["volume"].size == 0 and (r["ids"] == -1).all()
    w["fw"][2, 2, 2] = 0.0                          # a solid cell is never core
    _air(w, 2, 2, 2, lw=0.0)
    assert cases.run_ref(w, DX)["units"].size == 0
    w["fw"][2, 2, 2] = 0.5                          # half solid: half the air
    assert cases.run_ref(w, DX)["units"].tolist() == [U // 2]


@pytest.mark.parametrize("cell", [(0, 2, 2), (5, 2, 2), (2, 0, 2), (2, 4, 2), (2, 2, 0), (2, 2, 3)])
def test_an_open_flag_from_each_side(cell):
    w = cases.liquid_weights()
    _air(w, 2, 2, 2)                               # interior: closed
    assert cases.run_ref(w, DX)["open"].tolist() == [0]
    i, j, k = cell
    w = cases.liquid_weights()
    _air(w, i, j, k)
    assert cases.run_ref(w, DX)["open"].tolist() == [1]
    # a skin cell on the border does not open a pocket: only core cells count
    w = cases.liquid_weights()
    _air(w, 2, 2, 2)
    _air(w, 2, 2, 3, lw=0.75)
    r = cases.run_ref(w, DX)
    assert r["ids"][3, 2, 2] == 0 and r["open"].tolist() == [0]


def numbering_case():
    """a single cell at a low index, five cells in a row at a high one"""
    w = cases.liquid_weights()
    _air(w, 4, 1, 0)
    for i in range(5):
        _air(w, i, 3, 2)
    return w


def test_pockets_are_numbered_by_their_smallest_cell():
    r = cases.run_ref(numbering_case(), DX)
    assert r["cells"].tolist() == [1, 5] and r["units"].tolist() == [U, 5 * U] and r["open"].tolist() == [1, 1]
    assert r["ids"][0, 1, 4] == 0 and (r["ids"][2, 3, :5] == 1).all()


def test_the_mutants_fail_these_cases():
    r = cases.run_ref(split_pair(True), DX, mutant="closed_faces_link")
    assert r["units"].tolist() == [2 * U]                         # joined through the solid face: the first test catches it
    assert cases.run_ref(split_pair(False), DX, mutant="closed_faces_link")["units"].tolist() == [2 * U]
    r = cases.run_ref(numbering_case(), DX, mutant="number_by_size")
    assert r["cells"].tolist() == [5, 1] and r["ids"][0, 1, 4] == 1   # the numbering test catches it
    assert cases.run_ref(split_pair(True), DX, mutant="number_by_size")["units"].tolist() == [U, U]


def test_the_crafted_scenes_are_what_their_names_say():
    m = cases.serpentine_mask()
    assert m.sum() > 500 and all(m[16 * by:16 * by + 16, 16 * bx:16 * bx + 16].any() for by in range(3) for bx in range(3))
    n = m.astype(int)
    nbrs = np.zeros_like(n)
    nbrs[1:] += n[:-1]; nbrs[:-1] += n[1:]; nbrs[:, 1:] += n[:, :-1]; nbrs[:, :-1] += n[:, 1:]
    assert (nbrs[m] <= 2).all() and (nbrs[m] == 1).sum() == 2      # one cell wide: a path with two ends
    sc, _ = cases.checkerboard()
    assert (sc.surface > 0).sum() == 32 * 32 * 16 // 2

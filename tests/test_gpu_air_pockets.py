"""Air pockets on the GPU (ps_label_air_pockets ...): upload, label, setup, read the weight arrays the setup used, and compare every output
with the numpy restatement (air_pockets_ref.py) fed those arrays.  Ids, units, cells and open are integers and compared exactly; the
volume is compared bitwise with the restatement's expression.  No comparison has a tolerance."""
import os
import sys

import numpy as np
import pytest

import polystokes_amd
from polystokes_amd import _abi as abi
from polystokes_amd import _hip
from polystokes_amd import scenes

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import children  # noqa: E402
import air_pockets_cases as cases  # noqa: E402
import air_pockets_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(HERE)
RELEASE = os.path.join(ROOT, "polystokes_amd", "libpolystokes_hip_release.so")
_labelled = {}


def labelled(name):
    """upload -> label -> setup of scene `name` on a fresh context, once: what the calls returned, the arrays, and the restatement on the
    weights of that setup (shared, never modified)"""
    if name not in _labelled:
        sc, p = cases.SCENES[name]()
        s = polystokes_amd.Solver(0)
        s.upload(sc, p)
        k = s.label_air_pockets()
        after_label = s.memory_stats()
        vol, opn = s.air_pockets()
        ids = s.air_pocket_ids()
        arrays_before = cases.got(s)
        s.setup()
        want = cases.run_ref(cases.weights_of(s, sc), sc.dx)          # (ps_fields_in.dx is a double: the library sees sc.dx itself)
        out = {"sc": sc, "p": p, "k": k, "volume": vol, "open": opn, "ids": ids, "before": arrays_before, "after": cases.got(s),
               "passes": int(s.array("airPocketPasses")[0]), "want": want, "memory": after_label, "setup_lw": s.array("centerLiquidWeights")}
        s.close()
        _labelled[name] = out
    return _labelled[name]


def check_against_restatement(name):
    r = labelled(name)
    w, sc = r["want"], r["sc"]
    K = w["units"].size
    print(name, "K", r["k"], "passes", r["passes"], "units", w["units"][:4], "open", w["open"][:4])
    assert r["k"] == K
    assert r["ids"].dtype == np.int32 and np.array_equal(r["ids"], w["ids"])
    n_pockets, ids, units, cells, opn, vol = r["after"]
    assert n_pockets.tolist() == [K] and np.array_equal(ids.reshape(w["ids"].shape), w["ids"])
    assert units.dtype == np.int64 and np.array_equal(units, w["units"])
    assert np.array_equal(cells, w["cells"]) and np.array_equal(opn, w["open"])
    assert vol.dtype == np.float64 and vol.tobytes() == w["volume"].tobytes()
    assert r["volume"].tobytes() == w["volume"].tobytes() and np.array_equal(r["open"], w["open"])
    for a, b in zip(r["before"], r["after"]):                      # the setup kept the labels, array by array
        assert a.tobytes() == b.tobytes()
    assert r["memory"]["deferred_bytes"] == 0
    return r, w


def test_bubbles_three_pockets_one_open():
    r, w = check_against_restatement("bubbles")
    assert r["k"] == 3 and w["open"].sum() == 1 and w["open"][0] == 1          # the air above the pool holds cell (0, 16, 0): pocket 0
    assert (w["cells"][1:] > 20).all() and (w["units"] > 0).all()
    ids = w["ids"]
    assert len(set(ids[:, :, 15].ravel()) & set(ids[:, :, 16].ravel()) & {1, 2}) == 1   # one bubble lies on both sides of the box border x = 16
    assert ((ids >= 0) & (r["setup_lw"].reshape(ids.shape) > 0.5)).any()                # skin cells exist


@pytest.mark.parametrize("name", ["odd19", "odd7"])
def test_odd_sizes(name):
    r, w = check_against_restatement(name)
    assert r["k"] >= 1 and w["open"][0] == 1
    if name == "odd19":
        assert r["k"] == 3


def test_serpentine_needs_repeated_global_passes():
    r, w = check_against_restatement("serpentine")
    assert r["k"] == 2
    mask = cases.serpentine_mask()
    assert w["cells"][0] == mask.sum() and w["open"].tolist() == [0, 1]
    assert (w["ids"][8][mask] == 0).all() and (w["ids"][8][~mask] == -1).all()
    assert r["passes"] > 1


def test_many_pockets():
    r, w = check_against_restatement("checkerboard")
    assert r["k"] == 32 * 32 * 16 // 2 > 2000
    assert (w["cells"] == 1).all() and (w["units"] == 1048576).all()
    air = np.flatnonzero(w["ids"].ravel() >= 0)
    assert np.array_equal(w["ids"].ravel()[air], np.arange(air.size))          # numbered in x-fastest order across the scan's tiles


def test_a_workgroup_walks_several_tiles_and_a_wave_changes_its_pocket():
    """675 840 cells: the sum kernel's workgroups walk three tiles each, the last ones start beyond the grid; the two rooms alternate row by
    row along the walk (flush and reset of a wave's carried sums, tiles of mixed ids in between), the open air above is carried over
    whole runs"""
    r, w = check_against_restatement("two_rooms")
    sc = r["sc"]
    assert sc.nx * sc.ny * sc.nz > 1024 * 256 and sc.nx * sc.ny * sc.nz < 1024 * 3 * 256      # three tiles per workgroup, not all workgroups used
    assert r["k"] == 3 and w["open"].tolist() == [0, 0, 1]
    assert w["cells"].tolist() == [54 * 84 * 4, 56 * 84 * 4, 120 * 88 * 8]
    # a room's eight corner cells hold 7/8 of a cell: the sub-sample towards the corner is outvoted by its seven solid neighbours
    assert w["units"].tolist() == [(54 * 84 * 4 - 1) * 1048576, (56 * 84 * 4 - 1) * 1048576, 120 * 88 * 8 * 1048576]
    row = w["ids"][11, 40]
    assert set(row[2:56]) == {0} and set(row[62:118]) == {1} and set(row[56:62]) == {-1}      # both rooms in every row of the walk


def test_uploaded_weights_and_tied_skin_cells():
    """the caller's weights[14] are what the labelling reads; skin cells tied between two different pockets take the first direction"""
    sc, p = cases.tie_weights()
    s = polystokes_amd.Solver(0)
    s.upload(sc, p)
    k = s.label_air_pockets()
    ids = s.air_pocket_ids()
    got = cases.got(s)
    s.close()
    lw, fw, fwx, fwy, fwz = sc.weights[0], sc.weights[7], sc.weights[8], sc.weights[9], sc.weights[10]
    w = ref.pockets(lw, fw, fwx, fwy, fwz, sc.dx)
    assert k == w["units"].size == 11
    assert np.array_equal(ids, w["ids"])
    assert np.array_equal(got[2], w["units"]) and np.array_equal(got[3], w["cells"]) and np.array_equal(got[4], w["open"])
    assert got[5].tobytes() == w["volume"].tobytes()
    for skin, winner in (((2, 2, 1), (1, 2, 1)), ((6, 2, 1), (6, 1, 1)), ((9, 2, 2), (9, 2, 1)), ((2, 6, 4), (3, 6, 4)), ((7, 6, 4), (6, 6, 4)),
                         ((1, 8, 5), (1, 8, 6))):
        (i, j, kk), (a, b, c) = skin, winner
        assert ids[kk, j, i] == ids[c, b, a] >= 0, skin
    assert len({int(ids[1, 2, 1]), int(ids[1, 2, 3]), int(ids[1, 1, 6]), int(ids[1, 3, 6]), int(ids[1, 2, 9]), int(ids[3, 2, 9])}) == 6


def test_all_air_is_one_open_pocket():
    r, w = check_against_restatement("all_air")
    assert r["k"] == 1 and w["open"].tolist() == [1]
    assert w["units"].tolist() == [33 * 17 * 9 * 1048576] and w["cells"].tolist() == [33 * 17 * 9]


def test_all_liquid_has_no_pocket():
    r, w = check_against_restatement("all_liquid")
    assert r["k"] == 0 and r["volume"].size == 0 and r["open"].size == 0 and (r["ids"] == -1).all()
    for a in r["after"][2:]:
        assert a.size == 0
    sc, p = cases.all_liquid()
    s = polystokes_amd.Solver(0)
    s.upload(sc, p)
    assert s.label_air_pockets() == 0
    assert s.L.ps_get_air_pockets(s.h, None, None, 0) == abi.SUCCESS          # the getters succeed with len = 0
    assert s.set_air_pocket_pressures([]) == abi.SUCCESS
    assert s.set_air_pocket_pressures([1.0]) == abi.INVALID
    s.close()


def _step(s, sc, p, label=False, pressures=None, field=None, sigma=None):
    s.upload(sc, p)
    if sigma is not None or field is not None:
        assert s.upload_surface_fields(sigma, field) == abi.SUCCESS, s.last_error()
    if label:
        s.label_air_pockets()
    if pressures is not None:
        assert s.set_air_pocket_pressures(pressures) == abi.SUCCESS, s.last_error()
    rc = s.step_device()
    vel, valid = s.download()
    out = {"rc": rc, "vel": [v.copy() for v in vel], "valid": [v.copy() for v in valid], "it": int(s.stats.solveData[1]),
           "err": float(s.stats.solveData[0]), "fields": int(s.array("surfaceFields")[0])}
    if out["fields"]:
        out["q"] = s.array("surfaceGhostPressure")
    return out


def _same_step(a, b):
    assert a["rc"] == b["rc"] and a["it"] == b["it"] and np.float64(a["err"]).tobytes() == np.float64(b["err"]).tobytes()
    for q in range(3):
        assert a["vel"][q].tobytes() == b["vel"][q].tobytes() and a["valid"][q].tobytes() == b["valid"][q].tobytes()


_plain = {}


def plain_step():
    if not _plain:
        sc, p = cases.bubbles()
        s = polystokes_amd.Solver(0)
        _plain.update(_step(s, sc, p))
        s.close()
    return _plain


def test_labelling_does_not_change_a_step():
    sc, p = cases.bubbles()
    s = polystokes_amd.Solver(0)
    got = _step(s, sc, p, label=True)
    assert int(s.array("airPockets")[0]) == 3                        # ... and the step kept the labels
    assert np.array_equal(s.air_pocket_ids(), labelled("bubbles")["ids"])
    s.close()
    assert got["rc"] in (abi.SUCCESS, abi.NOCONVERGE) and got["it"] > 3 and got["fields"] == 0
    _same_step(plain_step(), got)


def test_pressures_reach_the_step_like_an_uploaded_field():
    sc, p = cases.bubbles()
    P = [0.0, 500.0, 2000.0]
    ids = labelled("bubbles")["ids"]
    field = ref.pressure_field(ids, P)
    assert set(np.unique(field).tolist()) == {0.0, 500.0, 2000.0}
    s = polystokes_amd.Solver(0)
    other = polystokes_amd.Solver(0)                     # a second context takes the numpy-built field: nothing of the first can reach it
    got = _step(s, sc, p, label=True, pressures=P)
    want = _step(other, sc, p, field=field)
    _same_step(want, got)
    assert got["fields"] == 2 and got["q"].tobytes() == want["q"].tobytes()
    assert any(got["vel"][q].tobytes() != plain_step()["vel"][q].tobytes() for q in range(3))      # the field is read
    # a sigma field that is present stays
    sigma = np.full(ids.shape, 0.07, np.float32)
    got = _step(s, sc, p, label=True, pressures=P, sigma=sigma)
    want = _step(other, sc, p, field=field, sigma=sigma)
    other.close()
    assert got["fields"] == 3
    _same_step(want, got)
    assert got["q"].tobytes() == want["q"].tobytes()
    # NULL drops the pressure member alone
    s.upload(sc, p)
    assert s.upload_surface_fields(sigma, None) == abi.SUCCESS
    s.label_air_pockets()
    assert s.set_air_pocket_pressures(P) == abi.SUCCESS and s.set_air_pocket_pressures(None) == abi.SUCCESS
    s.setup()
    assert int(s.array("surfaceFields")[0]) == 1
    s.close()


def test_pressure_refusals_change_nothing():
    sc, p = cases.bubbles()
    s = polystokes_amd.Solver(0)
    s.upload(sc, p)
    with pytest.raises(polystokes_amd.PolyStokesError, match="no air pocket labels"):
        s.set_air_pocket_pressures([0.0, 1.0, 2.0])
    assert s.label_air_pockets() == 3
    assert s.set_air_pocket_pressures([0.0, 1.0]) == abi.INVALID and "len must equal the pocket count 3" in s.last_error()
    assert s.set_air_pocket_pressures([0.0, 1.0, 2.0, 3.0]) == abi.INVALID
    assert s.set_air_pocket_pressures([0.0, float("nan"), float("inf")]) == abi.INVALID
    assert "pressure of pocket 1 is not finite" in s.last_error()
    # a finite double beyond fp32 would paint an infinity, which ps_upload_surface_fields refuses in the same array
    assert s.set_air_pocket_pressures([0.0, 1.0, 1e39]) == abi.INVALID and "pressure of pocket 2 is not finite" in s.last_error()
    with np.errstate(over="ignore"):
        field = ref.pressure_field(labelled("bubbles")["ids"], [0.0, 1.0, 1e39])
    assert np.isinf(field).any()
    assert s.upload_surface_fields(None, field) == abi.INVALID and "non-finite" in s.last_error()
    assert s.set_air_pocket_pressures([0.0, 1.0, 3.0e38]) == abi.SUCCESS and s.set_air_pocket_pressures(None) == abi.SUCCESS
    assert s.memory_stats()["deferred_bytes"] == 0
    s.setup()
    assert int(s.array("surfaceFields")[0]) == 0                     # nothing was installed
    s.close()


def test_lifetime():
    sc, p = cases.bubbles()
    s = polystokes_amd.Solver(0)
    fresh = polystokes_amd.Solver(0)
    assert fresh.L.ps_label_air_pockets(fresh.h, None) == abi.INVALID          # before any upload
    with pytest.raises(polystokes_amd.PolyStokesError, match="no air pocket labels"):
        fresh.air_pockets()
    one = np.zeros(1, np.int32)
    assert fresh.L.ps_download_air_pocket_ids(fresh.h, one.ctypes.data) == abi.FAILED and "no air pocket labels" in fresh.last_error()
    fresh.close()
    s.upload(sc, p)
    assert s.label_air_pockets() == 3
    first = cases.got(s) + list(s.air_pockets())
    live = s.memory_stats()["live_bytes"]
    for _ in range(9):
        assert s.label_air_pockets() == 3
    stats = s.memory_stats()
    assert stats["live_bytes"] == live and stats["deferred_bytes"] == 0        # ten calls hold what the first held
    again = cases.got(s) + list(s.air_pockets())
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(first, labelled("bubbles")["after"]):                      # ... and another context found the same
        assert a.tobytes() == b.tobytes()
    s.upload(sc, p)                                                            # a second upload drops the labels
    with pytest.raises(KeyError):
        s.array("airPockets")
    for call in (s.air_pockets, s.air_pocket_ids, lambda: s.set_air_pocket_pressures([0.0, 0.0, 0.0])):
        with pytest.raises(polystokes_amd.PolyStokesError, match="no air pocket labels"):
            call()
    dev = _hip.DeviceBuffer(sc.nx * sc.ny * sc.nz)
    with pytest.raises(polystokes_amd.PolyStokesError, match="no air pocket labels"):
        s.air_pocket_ids_device(dev, 0)
    assert s.memory_stats()["live_bytes"] < live                               # the id grid and the results were released
    s.close()


def test_a_decomposition_is_refused_and_drops_the_labels():
    sc, p, slab = scenes.cavity_slab(64, 2, 0, precond=abi.PRE_DIAGONAL)
    s = polystokes_amd.Solver(0)
    s.upload(sc, p)
    assert s.label_air_pockets() == 0
    s.set_slab(slab)
    with pytest.raises(KeyError):
        s.array("airPockets")
    with pytest.raises(polystokes_amd.PolyStokesError, match="air pockets need a single domain"):
        s.label_air_pockets()
    s.close()
    g = polystokes_amd.Group(2)
    g.ranks[0].upload(sc, p)
    with pytest.raises(polystokes_amd.PolyStokesError, match="air pockets need a single domain"):
        g.ranks[0].label_air_pockets()
    g.close()


def test_device_download_in_both_layouts():
    r = labelled("bubbles")
    sc, p = r["sc"], r["p"]
    n = sc.nx * sc.ny * sc.nz
    s = polystokes_amd.Solver(0)
    s.upload(sc, p)
    s.label_air_pockets()
    stream = _hip.Stream()
    for layout in (abi.LAYOUT_X_FASTEST, abi.LAYOUT_Z_FASTEST):
        dev = _hip.DeviceBuffer(n, pad=1)                                      # 4-byte aligned only: a view with a storage offset
        assert s.air_pocket_ids_device(dev, layout, stream) == abi.SUCCESS, s.last_error()
        stream.synchronize()
        flat = dev.to_numpy().view(np.int32)
        assert np.array_equal(polystokes_amd.from_layout(flat, r["ids"].shape, layout), r["ids"]), layout
        dev.close()
    small = _hip.DeviceBuffer(n - 1)
    assert s.air_pocket_ids_device(small, 0, stream) == abi.INVALID and "allocation ends before" in s.last_error()
    assert s.air_pocket_ids_device(small, 2, stream) == abi.INVALID and "layout" in s.last_error()
    host = np.zeros(n, np.int32)
    assert s.air_pocket_ids_device(host.ctypes.data, 0, stream) == abi.INVALID
    assert s.air_pocket_ids_device(None, 0, stream) == abi.INVALID
    small.close()
    stream.close()
    s.close()


def _child(name, env_extra, expect=()):
    pr = children.run_script("air_pockets_cases.py", "label", name, limit=600, env=env_extra, drop=("PS_LIB",), expect=expect)
    return " ".join(("DIGEST",) + pr.digests()[-1]), pr.output


def _digest(name):
    r = labelled(name)
    return "DIGEST %d %s" % (r["k"], cases.digest(r["after"] + [r["ids"], r["volume"], r["open"]]))


@pytest.mark.parametrize("name", ["bubbles", "serpentine"])
def test_poisoned_buffers_change_nothing(name):
    """PS_DEBUG_POISON=1 fills whatever a buffer allocation hands out with 0xff: a label, a flag or a sum nobody wrote would show"""
    line, _ = _child(name, {"PS_DEBUG_POISON": "1"}, expect=("PS_DEBUG_POISON=1 is active",))     # the child read the switch
    assert line == _digest(name)


def test_release_library_labels_the_same():
    assert os.path.exists(RELEASE), "build it: make -C polystokes_amd/csrc"
    line, _ = _child("bubbles", {"PS_LIB": RELEASE})
    assert line == _digest("bubbles")

"""Velocity extrapolation (ps_set_velocity_extrapolation) on the GPU.  The rule is a function of the step's own vel and valid and is restated
exactly in numpy (extrapolation_ref.py), so every comparison is on the bytes: the reference of a case is the rule applied to what a fresh
context WITHOUT the setting returns for the same scene (the step is deterministic: test_gpu_device_fields.py holds that control).
test_extrapolation_ref_cpu.py shows that these scenes tell the rule from its near misses."""
import os
import sys

import numpy as np
import pytest

import polystokes_amd
from polystokes_amd import _abi as abi
from polystokes_amd import scenes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import children  # noqa: E402
import device_fields_cases as dcases  # noqa: E402
import extrapolation_cases as cases  # noqa: E402
import extrapolation_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESSAGE = "layers outside 0..64"
_mode0, _want = {}, {}


def mode0(name):
    """One step of scene `name` on a fresh context that never made the call; computed once, shared, never modified."""
    if name not in _mode0:
        _mode0[name] = cases.fresh(name)
    return _mode0[name]


def want(name, layers):
    """The rule applied to mode0(name): (vel[3], L[3], counts summed over the axes)"""
    if (name, layers) not in _want:
        m = mode0(name)
        per_axis = [ref.extrapolate(m["vel"][a], m["valid"][a], layers) for a in range(3)]
        _want[(name, layers)] = ([r[0] for r in per_axis], [r[1] for r in per_axis], sum(r[2].astype(np.int64) for r in per_axis).astype(np.int32))
    return _want[(name, layers)]


def check(got, name, layers):
    m = mode0(name)
    vel, L, counts = want(name, layers)
    assert got["rc"] == m["rc"] and got["rc"] in (abi.SUCCESS, abi.NOCONVERGE) and got["iterations"] == m["iterations"] and got["x"] == m["x"]
    assert got["used"] == layers
    for a in range(3):
        assert got["valid"][a].tobytes() == m["valid"][a].tobytes(), a
        assert got["vel"][a].tobytes() == vel[a].tobytes(), (a, int((got["vel"][a].view(np.uint32) != vel[a].view(np.uint32)).sum()))
        assert got["layer"][a].dtype == np.int8 and np.array_equal(got["layer"][a], L[a]), a
    assert got["counts"].dtype == np.int32 and np.array_equal(got["counts"], counts), (got["counts"], counts)


# ---- 1. bit for bit ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", [1, 3, 12])
@pytest.mark.parametrize("name", ["blob0", "droplet24", "sliding32"])
def test_step_equals_the_rule_bit_for_bit(name, layers):
    got = cases.fresh(name, layers)
    check(got, name, layers)
    vel, L, counts = want(name, layers)
    m = mode0(name)
    assert counts[0] > 0 and any(vel[a].tobytes() != m["vel"][a].tobytes() for a in range(3))     # the case is not vacuous
    if name == "sliding32" and layers == 12:
        assert got["counts"][11] == 0 and np.all(got["counts"][:11] > 0), got["counts"]        # saturated: the last sweep finds nothing


# ---- 2. no-op scene ----------------------------------------------------------------------------------------------------------------------
def test_scene_without_invalid_faces_is_untouched():
    got = cases.fresh("cavity32", 4)
    m = mode0("cavity32")
    assert got["used"] == 4 and list(got["counts"]) == [0, 0, 0, 0]
    for a in range(3):
        assert got["vel"][a].tobytes() == m["vel"][a].tobytes() and got["valid"][a].tobytes() == m["valid"][a].tobytes()
        assert np.all(got["layer"][a] == 0)
    assert (got["rc"], got["iterations"], got["x"]) == (m["rc"], m["iterations"], m["x"])


# ---- 3. every path -----------------------------------------------------------------------------------------------------------------------
def test_every_entry_point_returns_the_extrapolated_velocity():
    name, layers = "blob0", 3
    sc, p = cases.scene(name)
    s = polystokes_amd.Solver(0)
    try:
        assert s.set_velocity_extrapolation(layers) == abi.SUCCESS
        # ps_upload_fields, ps_setup_device, ps_solve_device, ps_download_fields
        s.upload(sc, p)
        s.setup()
        rc = s.solve()
        s.download()
        check(cases.outcome(s, rc), name, layers)
        # polystokes_step
        check(cases.outcome(s, s.step(sc, p)), name, layers)
        # ps_step_device_fields and ps_download_fields_device, both layouts
        vel, _, _ = want(name, layers)
        m = mode0(name)
        for layout in (abi.LAYOUT_X_FASTEST, abi.LAYOUT_Z_FASTEST):
            ds = polystokes_amd.device_scene(sc, layout)
            rc, dv, dok = s.step_device_fields(p, ds, layout)
            assert rc == m["rc"], s.last_error()
            for source in ((dv, dok), s.download_device(layout)[1:]):
                v, ok = dcases.device_outputs(sc, source[0], source[1], layout)
                for a in range(3):
                    assert v[a].tobytes() == vel[a].tobytes(), (layout, a)
                    assert ok[a].tobytes() == m["valid"][a].tobytes(), (layout, a)
            assert int(s.array("velocityExtrapolation")[0]) == layers
    finally:
        s.close()


# ---- 4. velocity not written -------------------------------------------------------------------------------------------------------------
def _assert_nothing_ran(s, sc):
    assert int(s.array("velocityExtrapolation")[0]) == 0
    for n in cases.LAYER_ARRAYS + ("extrapolationCounts",):
        with pytest.raises(KeyError):
            s.array(n)
    for a in range(3):
        assert s.vel[a].tobytes() == sc.vel[a].tobytes(), a


def test_interrupted_step_leaves_the_input_velocity():
    sc, p = cases.scene("spheres32")
    s = polystokes_amd.Solver(0)
    try:
        assert s.set_velocity_extrapolation(4) == abi.SUCCESS
        s.set_interrupt(lambda: True)
        assert s.step(sc, p) == abi.INCOMPLETE
        s.set_interrupt(None)
        _assert_nothing_ran(s, sc)
    finally:
        s.close()


def test_dropped_nonconverged_step_leaves_the_input_velocity():
    sc, p = cases.scene("spheres32")
    p.maxSolverIterations, p.keepNonConvergedResults = 5, 0
    results = []
    for layers in (None, 4):
        s = polystokes_amd.Solver(0)
        try:
            if layers is not None:
                assert s.set_velocity_extrapolation(layers) == abi.SUCCESS
            rc = s.step(sc, p)
            assert rc == abi.NOCONVERGE
            _assert_nothing_ran(s, sc)
            results.append((rc, int(s.stats.solveData[1]), [v.tobytes() for v in s.vel], [v.tobytes() for v in s.valid]))
        finally:
            s.close()
    assert results[0] == results[1]


# ---- 5. Picard passes --------------------------------------------------------------------------------------------------------------------
def test_picard_passes_end_with_the_extrapolation_of_the_last_pass():
    layers = 3
    runs = []
    for setting in (None, layers):
        s = polystokes_amd.Solver(0)
        try:
            assert s.set_rheology(flow_index=0.7, passes=2, min_shear_rate=1e-2, min_viscosity=1e-3, max_viscosity=1e5) == abi.SUCCESS
            sc, p = scenes.blob()
            p.preconditioner = abi.PRE_DIAGONAL
            got = cases.step(s, sc, p, setting)
            got["passes"] = list(s.array("rheologyIterations"))
            runs.append(got)
        finally:
            s.close()
    base, got = runs
    assert base["rc"] == got["rc"] == abi.SUCCESS and len(base["passes"]) == 3 and got["passes"] == base["passes"]
    assert got["x"] == base["x"] and got["used"] == layers and base["used"] == 0
    for a in range(3):
        vel, L, _ = ref.extrapolate(base["vel"][a], base["valid"][a], layers)
        assert got["valid"][a].tobytes() == base["valid"][a].tobytes()
        assert got["vel"][a].tobytes() == vel.tobytes(), a
        assert np.array_equal(got["layer"][a], L)
        assert vel.tobytes() != base["vel"][a].tobytes()


# ---- 6. mode 0 is untouched --------------------------------------------------------------------------------------------------------------
def test_setting_zero_after_steps_with_it_equals_a_fresh_context():
    name = "blob0"
    sc, p = cases.scene(name)
    m = mode0(name)
    s = polystokes_amd.Solver(0)
    try:
        check(cases.step(s, sc, p, 3), name, 3)
        check(cases.step(s, sc, p, 12), name, 12)
        got = cases.step(s, sc, p, 0)
        assert got["used"] == 0 and got["layer"] is None and got["counts"] is None
        assert (got["rc"], got["iterations"], got["x"]) == (m["rc"], m["iterations"], m["x"])
        for a in range(3):
            assert got["vel"][a].tobytes() == m["vel"][a].tobytes() and got["valid"][a].tobytes() == m["valid"][a].tobytes()
    finally:
        s.close()


def test_memory_is_flat_and_released_with_the_setting():
    sc, p = cases.scene("blob0")
    s = polystokes_amd.Solver(0)
    try:
        s.upload(sc, p)
        s.step_device()
        s.step_device()
        base = s.memory_stats()["live_bytes"]
        assert s.set_velocity_extrapolation(4) == abi.SUCCESS
        assert s.memory_stats()["live_bytes"] == base                  # the setting alone allocates nothing
        seen = []
        for _ in range(4):
            assert s.step_device() == abi.SUCCESS and int(s.array("velocityExtrapolation")[0]) == 4
            mem = s.memory_stats()
            assert mem["deferred_bytes"] == 0
            seen.append(mem["live_bytes"])
        assert len(set(seen)) == 1, seen
        nx, ny, nz = sc.nx, sc.ny, sc.nz
        faces = (nx + 1) * ny * nz + nx * (ny + 1) * nz + nx * ny * (nz + 1)
        assert seen[0] - base == faces + 4 * abi.EXTRAPOLATION_MAX_LAYERS, (seen[0] - base, faces)     # include/polystokes.h: 1 B per face + 256
        assert s.set_velocity_extrapolation(0) == abi.SUCCESS
        mem = s.memory_stats()
        assert mem["deferred_bytes"] == 0 and mem["live_bytes"] == base
        with pytest.raises(KeyError):
            s.array("extrapolationLayerX")
    finally:
        s.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------
def test_values_outside_the_range_are_refused_and_keep_the_setting():
    name = "blob0"
    sc, p = cases.scene(name)
    s = polystokes_amd.Solver(0)
    try:
        assert s.set_velocity_extrapolation(3) == abi.SUCCESS
        for bad in (-1, 65, 1000):
            assert s.set_velocity_extrapolation(bad) == abi.INVALID
            assert MESSAGE in s.last_error(), s.last_error()
        check(cases.step(s, sc, p), name, 3)                           # the previous setting held
        assert s.set_velocity_extrapolation(abi.EXTRAPOLATION_MAX_LAYERS) == abi.SUCCESS
    finally:
        s.close()


# ---- 8. ignored on decompositions --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [None, (2, 1, 1)])
def test_in_process_groups_ignore_the_setting(dims):
    sc, p = cases.scene("cavity32t8")
    runs = []
    for layers in (None, 4):
        g = polystokes_amd.Group(2, dims=dims)
        try:
            if layers is not None:
                assert g.set_velocity_extrapolation(layers) == abi.SUCCESS
            rc = g.solve_scene(sc, p)
            for r in g.ranks:
                assert int(r.array("velocityExtrapolation")[0]) == 0
                with pytest.raises(KeyError):
                    r.array("extrapolationLayerX")
            runs.append((rc, int(g.stats.solveData[1]), [v.tobytes() for v in g.vel], [v.tobytes() for v in g.valid],
                         [r.array("solutionVector").tobytes() for r in g.ranks]))
        finally:
            g.close()
    assert runs[0][0] == abi.SUCCESS and runs[0] == runs[1]


def _slab_pair(layers, tmp_path):
    """two processes, one slab rank each, over the host-staged TCP transport (ps_step_device -> the distributed step)"""
    base = children.free_port_base(2)
    outs = [str(tmp_path / ("slab%d.r%d.npz" % (layers, r))) for r in range(2)]
    children.run_group([children.script_argv("extrapolation_cases.py", "slab", layers, r, base, outs[r]) for r in range(2)], limit=240, drop=("PS_LIB",))
    return [np.load(o) for o in outs]


def test_a_slab_pair_of_processes_ignores_the_setting(tmp_path):
    plain, withit = _slab_pair(-1, tmp_path), _slab_pair(4, tmp_path)       # -1: the ranks never make the call
    for r in range(2):
        assert int(withit[r]["used"]) == 0 and int(withit[r]["has_layer"]) == 0
        assert int(plain[r]["rc"]) == int(withit[r]["rc"]) == abi.SUCCESS and int(plain[r]["iterations"]) == int(withit[r]["iterations"])
        for a in range(3):
            assert plain[r]["vel%d" % a].tobytes() == withit[r]["vel%d" % a].tobytes(), (r, a)
            assert plain[r]["valid%d" % a].tobytes() == withit[r]["valid%d" % a].tobytes(), (r, a)


# ---- 9. child processes ------------------------------------------------------------------------------------------------------------------
def _child_digest(name, layers, env_extra, expect=()):
    pr = children.run_script("extrapolation_cases.py", "step", name, layers, limit=600, env=env_extra, drop=("PS_LIB",), expect=expect)
    lines = pr.digests()
    assert len(lines) == 1, pr.output[-2000:]
    return lines[0][0], pr.output


def _want_digest(name, layers):
    vel, L, counts = want(name, layers)
    return cases.digest(vel, mode0(name)["valid"], L, counts, layers)


def test_poisoned_buffers_change_nothing():
    """PS_DEBUG_POISON=1 fills whatever a buffer allocation hands out with 0xff: a sweep that read layer bytes nobody wrote would show"""
    got, _ = _child_digest("blob0", 3, {"PS_DEBUG_POISON": "1"}, expect=("PS_DEBUG_POISON=1 is active",))   # the child read the switch
    assert got == _want_digest("blob0", 3)


def test_release_library_extrapolates():
    rel = os.path.join(ROOT, "polystokes_amd", "libpolystokes_hip_release.so")
    assert os.path.exists(rel), "build it: make -C polystokes_amd/csrc"
    got, _ = _child_digest("blob0", 3, {"PS_LIB": rel})
    assert got == _want_digest("blob0", 3)


# ---- 10. determinism ---------------------------------------------------------------------------------------------------------------------
def test_two_steps_on_one_context_are_identical():
    sc, p = cases.scene("sliding32")
    s = polystokes_amd.Solver(0)
    try:
        first = cases.step(s, sc, p, 12)
        second = cases.step(s, sc, p)
        check(first, "sliding32", 12)
        check(second, "sliding32", 12)
    finally:
        s.close()

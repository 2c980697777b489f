"""The advection schemes (ps_advect_fields_scheme, ps_advect_fields_scheme_device) on the GPU.  With the MacCormack correction the outputs,
the counters of both passes and the step factor are a function of the grid, dx, dt, the order, the limiter, the carrier and the fields,
restated in numpy (advection_scheme_ref.py): the device is compared with the restatement byte for byte on the shared cases
(advection_scheme_cases.py); test_advection_scheme_ref_cpu.py shows that those cases tell the rule from its near misses.  With scheme 0 the
call is ps_advect_fields.  No test provokes a fault: every index the rule forms is clamped before it is used, and a refused call launches
nothing."""
import ctypes
import os
import sys

import numpy as np
import pytest

import polystokes_amd
from polystokes_amd import _abi as abi
from polystokes_amd import _hip
from polystokes_amd import from_layout, to_layout

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import children  # noqa: E402
import advection_cases as plain  # noqa: E402
import advection_scheme_cases as cases  # noqa: E402
import advection_scheme_ref as sref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELEASE = os.path.join(ROOT, "polystokes_amd", "libpolystokes_hip_release.so")
MAC = abi.ADVECT_MACCORMACK
SENTINEL = np.float32(-12345.5)


def uploaded(grid):
    s = polystokes_amd.Solver(0)
    s.upload(*cases.scene(grid))
    return s


class OnDevice:
    """a case's arrays on the device in one layout, outputs filled with the sentinel; pad: a storage offset of 4 bytes on cellIn[0]"""

    def __init__(self, grid, car, fields, layout, velocity=True, pad=0):
        self.layout, self.dims = layout, cases.GRIDS[grid]
        nx, ny, nz = self.dims
        self.cell_shape, self.face_shapes = (nz, ny, nx), cases.face_shapes(self.dims)
        put = lambda a, p=0: _hip.DeviceBuffer.from_numpy(to_layout(a, layout), p)
        blank = lambda shape: _hip.DeviceBuffer.from_numpy(np.full(int(np.prod(shape)), SENTINEL, np.float32))
        self.car = None if car is None else [put(c) for c in car]
        self.cin = [put(f, pad if q == 0 else 0) for q, f in enumerate(fields)]
        self.cout = [blank(self.cell_shape) for _ in fields]
        self.vout = [blank(sh) for sh in self.face_shapes] if velocity else None

    def outputs(self):
        cells = [from_layout(b.to_numpy(), self.cell_shape, self.layout) for b in self.cout]
        vel = None if self.vout is None else [from_layout(b.to_numpy(), sh, self.layout) for b, sh in zip(self.vout, self.face_shapes)]
        return cells, vel

    def untouched(self):
        return all((b.to_numpy() == SENTINEL).all() for b in self.cout + (self.vout or []))

    def close(self):
        for b in (self.car or []) + self.cin + self.cout + (self.vout or []):
            b.close()


def assert_same(got, want, what):
    """(cell outputs, velocity outputs or None, counts, r, correction) byte for byte"""
    print(what, "counts device", np.asarray(got[2]).tolist(), "reference", np.asarray(want[2]).tolist(), "correction device", np.asarray(got[4]).tolist(),
          "reference", np.asarray(want[4]).tolist())
    assert np.array_equal(np.asarray(got[2], np.int32), want[2]), what
    assert np.array_equal(np.asarray(got[4], np.int32), want[4]), what
    assert np.float64(got[3]).tobytes() == np.float64(want[3]).tobytes(), what
    assert len(got[0]) == len(want[0]) and (got[1] is None) == (want[1] is None), what
    for name, a, b in [("cell %d" % q, a, b) for q, (a, b) in enumerate(zip(got[0], want[0]))] + \
                      [("vel %d" % q, a, b) for q, (a, b) in enumerate(zip(got[1] or [], want[1] or []))]:
        bad = np.argwhere(np.asarray(a).view(np.uint32) != b.view(np.uint32))
        assert bad.size == 0, (what, name, len(bad), bad[:4].tolist())


# ---- 1. against the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", sorted(cases.GRIDS))
@pytest.mark.parametrize("kind", cases.CARRIERS)
def test_host_form_equals_the_restatement(grid, kind):
    s = uploaded(grid)
    try:
        for order in (1, 2):
            for limiter in cases.LIMITERS:
                assert_same(cases.run_host(s, grid, kind, order, limiter), cases.reference(grid, kind, order, limiter), "%s %s order %d limiter %d" % (grid, kind, order, limiter))
                assert int(s.array("advection")[0]) == order and s.array("advectionScheme").tolist() == [MAC, limiter]
                assert s.memory_stats()["deferred_bytes"] == 0
    finally:
        s.close()


@pytest.mark.parametrize("grid", sorted(cases.GRIDS))
@pytest.mark.parametrize("layout", (abi.LAYOUT_X_FASTEST, abi.LAYOUT_Z_FASTEST))
def test_device_form_in_both_layouts_equals_the_restatement(grid, layout):
    """device arrays behind a caller's stream, one input pointer 4 bytes into its allocation; the reference is the same for both layouts"""
    s = uploaded(grid)
    stream = _hip.Stream()
    try:
        for kind, order, limiter in (("gentle", 2, 1), ("nonfinite", 1, 2), ("negative_dt", 2, 0), ("random", 2, 2)):
            car, dt = cases.carrier(grid, kind)
            d = OnDevice(grid, car, cases.cell_fields(grid), layout, pad=1)
            assert d.cin[0].ptr % 8 == 4
            rc = s.advect_device(dt, d.cin, d.cout, order=order, carrier=d.car, vel_out=d.vout, layout=layout, stream=stream, scheme=MAC, limiter=limiter)
            assert rc == abi.SUCCESS, s.last_error()
            stream.synchronize()                                                   # the stream waits for the result; the host for the stream
            assert_same(d.outputs() + cases.what_the_call_left(s), cases.reference(grid, kind, order, limiter), "%s %s layout %d" % (grid, kind, layout))
            d.close()
    finally:
        stream.close()
        s.close()


@pytest.mark.parametrize("grid", sorted(cases.GRIDS))
@pytest.mark.parametrize("layers", (0, 3))
def test_the_contexts_carrier_is_the_downloaded_velocity(grid, layers):
    """carrier all NULL: the reference is computed from what ps_download_fields returns after the step, with and without extrapolation"""
    sc, p = cases.scene(grid)
    s = polystokes_amd.Solver(0)
    try:
        assert s.set_velocity_extrapolation(layers) == abi.SUCCESS
        s.upload(sc, p)
        s.step_device()
        vel, valid = s.download()
        dt = plain.stepped_dt(sc, vel) / 3.7 * 1.3                                 # max|u| dt / dx = 1.3: most samples are corrected
        fields = cases.cell_fields(grid)
        for order, limiter in ((1, 1), (2, 2)):
            want = sref.advect(cases.GRIDS[grid], float(sc.dx), dt, order, vel, fields, True, limiter)
            rc, cout, vout = s.advect(dt, fields, order=order, carrier=None, velocity=True, scheme=MAC, limiter=limiter)
            assert rc == abi.SUCCESS, s.last_error()
            assert_same((cout, vout) + cases.what_the_call_left(s), want, "%s layers %d order %d host" % (grid, layers, order))
            d = OnDevice(grid, None, fields, abi.LAYOUT_Z_FASTEST)
            rc = s.advect_device(dt, d.cin, d.cout, order=order, carrier=None, vel_out=d.vout, layout=d.layout, scheme=MAC, limiter=limiter)
            assert rc == abi.SUCCESS, s.last_error()
            assert_same(d.outputs() + cases.what_the_call_left(s), want, "%s layers %d order %d device" % (grid, layers, order))
            d.close()
    finally:
        s.close()


def test_eight_fields_in_one_call_equal_eight_calls_of_one():
    grid = "blob"
    base = cases.cell_fields(grid)
    fields = base + [np.float32(2.5) * base[0], base[1][::-1].copy(), -base[2], base[0] + base[2], np.sqrt(np.abs(base[1]))]
    assert len(fields) == abi.ADVECT_MAX_CELL_FIELDS
    car, dt = cases.carrier(grid, "gentle")
    s = uploaded(grid)
    try:
        rc, together, _ = s.advect(dt, fields, order=2, carrier=car, scheme=MAC, limiter=1)
        assert rc == abi.SUCCESS, s.last_error()
        left = cases.what_the_call_left(s)
        changed = 0
        for q, f in enumerate(fields):
            rc, one, _ = s.advect(dt, [f], order=2, carrier=car, scheme=MAC, limiter=1)
            assert rc == abi.SUCCESS and one[0].tobytes() == together[q].tobytes(), q
            n = s.array("advectionCorrection")
            assert np.array_equal(s.array("advectionCounts"), left[0]) and n[4] == left[2][4]     # a cell falls back once, whatever the number of fields
            changed += int(n[0])
        assert changed == int(left[2][0]) > 0                                      # ... and counts once per field the limiter changed
        want = sref.advect(cases.GRIDS[grid], float(cases.scene(grid)[0].dx), dt, 2, car, fields, False, 1)
        assert_same((together, None) + left, want, "eight fields")
    finally:
        s.close()


def test_velocity_alone_and_cell_fields_alone():
    grid = "odd"
    car, dt = cases.carrier(grid, "gentle")
    s = uploaded(grid)
    try:
        rc, cout, vout = s.advect(dt, (), order=2, carrier=car, velocity=True, scheme=MAC, limiter=2)
        assert rc == abi.SUCCESS and cout == [], s.last_error()
        assert_same(([], vout) + cases.what_the_call_left(s), cases.reference(grid, "gentle", 2, 2, fields=0, velocity=True), "velocity alone")
        rc, cout, vout = s.advect(dt, cases.cell_fields(grid), order=2, carrier=car, velocity=False, scheme=MAC, limiter=2)
        assert rc == abi.SUCCESS and vout is None, s.last_error()
        assert_same((cout, None) + cases.what_the_call_left(s), cases.reference(grid, "gentle", 2, 2, fields=3, velocity=False), "cell fields alone")
    finally:
        s.close()


def test_two_calls_on_one_context_give_identical_bytes():
    grid = "blob"
    s = uploaded(grid)
    try:
        first = cases.run_host(s, grid, "random", 2, 1)
        second = cases.run_host(s, grid, "random", 2, 1)
        assert cases.digest(*first) == cases.digest(*second) == cases.digest(*cases.reference(grid, "random", 2, 1))
    finally:
        s.close()


# ---- 2. scheme 0 is ps_advect_fields; the call changes nothing ----------------------------------------------------------------------------
def test_scheme_zero_is_the_semi_lagrangian_call():
    grid = "blob"
    car, dt = cases.carrier(grid, "random")
    fields = cases.cell_fields(grid)
    outcomes = []
    for scheme in (None, abi.ADVECT_SEMI_LAGRANGIAN):
        s = uploaded(grid)
        try:
            base = s.memory_stats()["live_bytes"]
            rc, cout, vout = s.advect(dt, fields, order=2, carrier=car, velocity=True, scheme=scheme, limiter=abi.ADVECT_LIMIT_REVERT)
            assert rc == abi.SUCCESS, s.last_error()
            d = OnDevice(grid, car, fields, abi.LAYOUT_Z_FASTEST)
            assert s.advect_device(dt, d.cin, d.cout, order=2, carrier=d.car, vel_out=d.vout, layout=d.layout, scheme=scheme) == abi.SUCCESS, s.last_error()
            _hip.rt().hipStreamSynchronize(None)
            mem = s.memory_stats()
            assert mem["live_bytes"] == base + 20 and mem["deferred_bytes"] == 0, (base, mem)
            for name in ("advectionScheme", "advectionCorrection"):
                with pytest.raises(KeyError):
                    s.array(name)                                                  # no new array
            outcomes.append(plain.digest(cout, vout, s.array("advectionCounts"), float(s.array("advectionStep")[0])) + plain.digest(*d.outputs(), s.array("advectionCounts"), 0.0))
            d.close()
        finally:
            s.close()
    assert outcomes[0] == outcomes[1]
    assert outcomes[0].startswith(plain.digest(*plain.reference(grid, "random", 2)))


def test_a_step_after_the_call_equals_a_step_without_it():
    grid = "blob"
    sc, p = cases.scene(grid)
    outcomes = []
    for call in (False, True):
        s = polystokes_amd.Solver(0)
        try:
            s.upload(sc, p)
            s.step_device()
            if call:
                rc, cout, vout = s.advect(3.0 * float(sc.dt), cases.cell_fields(grid), order=2, velocity=True, scheme=MAC, limiter=1)
                assert rc == abi.SUCCESS, s.last_error()
            rc = s.step_device()
            s.download()
            outcomes.append((int(rc), int(s.stats.solveData[1]), [v.tobytes() for v in s.vel], [v.tobytes() for v in s.valid], s.array("solutionVector").tobytes()))
            if call:
                assert s.array("advectionScheme").tolist() == [MAC, 1] and s.array("advectionCorrection").size == 8      # a step keeps the arrays
        finally:
            s.close()
    assert outcomes[0][1] > 0 and outcomes[0] == outcomes[1]


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing_and_register_nothing():
    grid = "odd"
    sc, p = cases.scene(grid)
    car, dt = cases.carrier(grid, "gentle")
    fields = cases.cell_fields(grid)
    s = polystokes_amd.Solver(0)
    try:
        d = OnDevice(grid, car, fields, abi.LAYOUT_X_FASTEST)
        host_out = [np.full(f.shape, SENTINEL, np.float32) for f in fields]
        host_vel = [np.full(c.shape, SENTINEL, np.float32) for c in car]
        good = abi.AdvectionScheme(MAC, abi.ADVECT_LIMIT_CLAMP)

        def both(S, why, rc=abi.INVALID, **kw):
            """the same refusal from both forms, nothing written"""
            args = dict(dt=dt, order=2, cell_in=fields, cell_out=host_out, carrier=car, vel_out=host_vel)
            dargs = dict(dt=dt, order=2, cell_in=d.cin, cell_out=d.cout, carrier=d.car, vel_out=d.vout)
            for k, (hv, dv) in kw.items():
                args[k], dargs[k] = hv, dv
            ref_s = None if S is None else ctypes.byref(S)
            got = s.L.ps_advect_fields_scheme(s.h, ctypes.byref(s.advection(**args)), ref_s)
            assert got == rc and why in s.last_error() and "PS_" not in s.last_error(), ("host", why, got, s.last_error())
            got = s.L.ps_advect_fields_scheme_device(s.h, ctypes.byref(s.advection(**dargs)), ref_s, 0, None)
            assert got == rc and why in s.last_error() and "PS_" not in s.last_error(), ("device", why, got, s.last_error())
            assert d.untouched() and all((o == SENTINEL).all() for o in host_out + host_vel), why

        both(good, "call ps_upload_fields first")
        s.upload(sc, p)
        base = s.memory_stats()["live_bytes"]
        assert s.L.ps_advect_fields_scheme(s.h, None, ctypes.byref(good)) == abi.INVALID and "a is null" in s.last_error()
        both(None, "s is null")
        for bad in (-1, 2):
            both(abi.AdvectionScheme(bad, 1), "scheme outside 0..1")
        for scheme in (0, 1):
            for bad in (-1, 3):
                both(abi.AdvectionScheme(scheme, bad), "limiter outside 0..2")     # validated with scheme 0 too
        for scheme in (0, 1):                                                      # the refusals of ps_advect_fields, in its words
            S = abi.AdvectionScheme(scheme, 1)
            both(S, "order outside 1..2", order=(3, 3))
            both(S, "dt not finite", dt=(np.nan, np.nan))
            both(S, "nothing to do", cell_in=((), ()), cell_out=((), ()), vel_out=(None, None))
            both(S, "no written velocity since the upload", rc=abi.FAILED, carrier=(None, None))
            A = s.advection(dt, 2, d.cin, d.cout, d.car, d.vout)
            assert s.L.ps_advect_fields_scheme_device(s.h, ctypes.byref(A), ctypes.byref(S), 2, None) == abi.INVALID and "layout must be 0" in s.last_error()
            A = s.advection(dt, 2, d.cin, [d.cin[0]] + d.cout[1:], d.car, d.vout)
            assert s.L.ps_advect_fields_scheme_device(s.h, ctypes.byref(A), ctypes.byref(S), 0, None) == abi.INVALID and "output 0 overlaps input 3" in s.last_error()
            A = s.advection(dt, 2, d.cin, d.cout, d.car, d.vout)
            A.cellOut[0] = host_out[0].ctypes.data
            assert s.L.ps_advect_fields_scheme_device(s.h, ctypes.byref(A), ctypes.byref(S), 0, None) == abi.INVALID and "cellOut: the pointer is not device memory" in s.last_error()
        assert d.untouched() and all((o == SENTINEL).all() for o in host_out + host_vel)
        for name in ("advection", "advectionCounts", "advectionScheme", "advectionCorrection"):
            with pytest.raises(KeyError):
                s.array(name)                                                      # no refused call registered anything
        mem = s.memory_stats()
        assert mem["live_bytes"] == base and mem["deferred_bytes"] == 0, (base, mem)                 # ... or allocated anything
        assert s.advect_device(dt, d.cin, d.cout, order=2, carrier=d.car, vel_out=d.vout, scheme=MAC, limiter=1) == abi.SUCCESS, s.last_error()
        assert_same(d.outputs() + cases.what_the_call_left(s), cases.reference(grid, "gentle", 2, 1), "after the refusals")
        d.close()
    finally:
        s.close()


# ---- 4. memory -------------------------------------------------------------------------------------------------------------------------------
def test_memory_is_as_stated_flat_and_gone_after_the_upload():
    grid = "blob"
    sc, p = cases.scene(grid)
    car, dt = cases.carrier(grid, "gentle")
    fields = cases.cell_fields(grid)
    nc, nf = fields[0].size, sum(c.size for c in car)
    s = uploaded(grid)
    try:
        base = s.memory_stats()["live_bytes"]
        d = OnDevice(grid, car, fields, abi.LAYOUT_X_FASTEST)                      # (the harness's own allocations are not the library's)

        def device(cell, vel):
            rc = s.advect_device(dt, d.cin[:cell], d.cout[:cell], order=2, carrier=d.car, vel_out=d.vout if vel else None, scheme=MAC, limiter=1)
            assert rc == abi.SUCCESS, s.last_error()
            _hip.rt().hipStreamSynchronize(None)
            return s.memory_stats()

        cases.run_host(s, grid, "gentle", 2, 1)
        mem = s.memory_stats()
        assert mem["live_bytes"] == base + 20 + 32 and mem["deferred_bytes"] == 0, (base, mem)       # the host form keeps the counters alone
        full = base + 20 + 32 + 4 * (3 * nc + nf)
        assert device(3, True)["live_bytes"] == full
        seen = []
        for call in range(4):                                                      # the largest call so far: nothing smaller or equal allocates
            if call % 2:
                mem = device(3 - call // 2, call == 1)
            else:
                cases.run_host(s, grid, "gentle", 2, 1)
                mem = s.memory_stats()
            assert mem["deferred_bytes"] == 0
            seen.append(mem["live_bytes"])
        assert seen == [full] * 4, (base, full, seen)
        s.upload(sc, p)
        mem = s.memory_stats()
        assert mem["live_bytes"] == base and mem["deferred_bytes"] == 0, (base, mem)
        for name in ("advection", "advectionStep", "advectionCounts", "advectionScheme", "advectionCorrection"):
            with pytest.raises(KeyError):
                s.array(name)
        d.close()
    finally:
        s.close()


# ---- 5. other builds and switches, each in a process of its own ---------------------------------------------------------------------------
CHILD_CASES = ("blob:gentle:2:1", "odd:nonfinite:1:2", "odd:random:2:0", "blob:negative_dt:1:2")


def _child(env, expect=()):
    pr = children.run_script("advection_scheme_cases.py", "advect", *CHILD_CASES, limit=300, env=env, drop=() if "PS_LIB" in env else ("PS_LIB",), expect=expect)
    want = {}
    for name in CHILD_CASES:
        grid, kind, order, limiter = name.split(":")
        want[name] = cases.digest(*cases.reference(grid, kind, int(order), int(limiter)))
    assert dict(pr.digests()) == want, pr.output[-2000:]


def test_poisoned_buffers_change_nothing():
    """PS_DEBUG_POISON=1 fills whatever a buffer allocation hands out with 0xff: a kernel that read a word of hat nobody wrote would show"""
    _child({"PS_DEBUG_POISON": "1"}, expect=["PS_DEBUG_POISON=1 is active"])


def test_the_release_library_gives_the_same_bytes():
    _child({"PS_LIB": RELEASE})

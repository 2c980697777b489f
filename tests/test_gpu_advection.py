"""Advection (ps_advect_fields, ps_advect_fields_device) on the GPU.  The outputs, the counters and the step factor are a function of the
grid, dx, dt, the order, the carrier and the fields, restated in numpy (advection_ref.py): the device is compared with the restatement byte
for byte on the shared cases (advection_cases.py).  test_advection_ref_cpu.py shows that those cases tell the rule from its near misses.
No test provokes a fault: every index the rule forms is clamped before it is used, and a refused call launches nothing."""
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
import advection_cases as cases  # noqa: E402
import advection_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELEASE = os.path.join(ROOT, "polystokes_amd", "libpolystokes_hip_release.so")
SENTINEL = np.float32(-12345.5)


def assert_same(got, want, what):
    """(cell outputs, velocity outputs or None, counts, r) byte for byte"""
    print(what, "counts device", np.asarray(got[2]).tolist(), "reference", np.asarray(want[2]).tolist(), "r", got[3], want[3])
    assert np.array_equal(np.asarray(got[2], np.int32), want[2]), what
    assert np.float64(got[3]).tobytes() == np.float64(want[3]).tobytes(), what
    assert len(got[0]) == len(want[0]) and (got[1] is None) == (want[1] is None), what
    for name, a, b in [("cell %d" % q, a, b) for q, (a, b) in enumerate(zip(got[0], want[0]))] + \
                      [("vel %d" % q, a, b) for q, (a, b) in enumerate(zip(got[1] or [], want[1] or []))]:
        bad = np.argwhere(np.asarray(a).view(np.uint32) != b.view(np.uint32))
        assert bad.size == 0, (what, name, len(bad), bad[:4].tolist())


def uploaded(grid):
    s = polystokes_amd.Solver(0)
    s.upload(*cases.scene(grid))
    return s


def counts_and_step(s):
    return s.array("advectionCounts"), float(s.array("advectionStep")[0])


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


# ---- 1. against the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", sorted(cases.GRIDS))
@pytest.mark.parametrize("kind", cases.CARRIERS)
def test_host_form_with_the_callers_carrier_equals_the_restatement(grid, kind):
    s = uploaded(grid)                                                             # no step: the caller's carrier needs none
    try:
        for order in (1, 2):
            assert_same(cases.run_host(s, grid, kind, order), cases.reference(grid, kind, order), "%s %s order %d" % (grid, kind, order))
            assert int(s.array("advection")[0]) == order
            assert s.memory_stats()["deferred_bytes"] == 0
    finally:
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
        assert int(s.array("velocityExtrapolation")[0]) == layers
        assert all(np.isfinite(v).all() for v in vel) and any((v != np.asarray(u, np.float32).reshape(v.shape)).any() for v, u in zip(vel, sc.vel))
        dt = cases.stepped_dt(sc, vel)
        fields = cases.cell_fields(grid)
        for order in (1, 2):
            want = ref.advect(cases.GRIDS[grid], float(sc.dx), dt, order, vel, fields, True)
            rc, cout, vout = s.advect(dt, fields, order=order, carrier=None, velocity=True)
            assert rc == abi.SUCCESS, s.last_error()
            assert_same((cout, vout) + counts_and_step(s), want, "%s layers %d order %d host" % (grid, layers, order))
            d = OnDevice(grid, None, fields, abi.LAYOUT_Z_FASTEST)
            assert s.advect_device(dt, d.cin, d.cout, order=order, carrier=None, vel_out=d.vout, layout=d.layout) == abi.SUCCESS, s.last_error()
            assert_same(d.outputs() + counts_and_step(s), want, "%s layers %d order %d device" % (grid, layers, order))
            d.close()
        assert abs(want[3] * max(float(np.abs(v).max()) for v in vel) - 3.7) < 1e-3
    finally:
        s.close()


@pytest.mark.parametrize("grid", sorted(cases.GRIDS))
@pytest.mark.parametrize("layout", (abi.LAYOUT_X_FASTEST, abi.LAYOUT_Z_FASTEST))
def test_device_form_in_both_layouts_equals_the_restatement(grid, layout):
    """device arrays behind a caller's stream, one input pointer 4 bytes into its allocation; the reference is the same for both layouts"""
    s = uploaded(grid)
    stream = _hip.Stream()
    try:
        for kind, order in (("random", 2), ("nonfinite", 1), ("negative_dt", 2)):
            car, dt = cases.carrier(grid, kind)
            d = OnDevice(grid, car, cases.cell_fields(grid), layout, pad=1)
            assert d.cin[0].ptr % 8 == 4
            assert s.advect_device(dt, d.cin, d.cout, order=order, carrier=d.car, vel_out=d.vout, layout=layout, stream=stream) == abi.SUCCESS, s.last_error()
            stream.synchronize()                                                   # the stream waits for the result; the host for the stream
            assert_same(d.outputs() + counts_and_step(s), cases.reference(grid, kind, order), "%s %s layout %d" % (grid, kind, layout))
            assert s.memory_stats()["deferred_bytes"] == 0
            d.close()
    finally:
        stream.close()
        s.close()


def test_eight_fields_in_one_call_equal_eight_calls_of_one():
    grid = "blob"
    base = cases.cell_fields(grid)
    fields = base + [np.float32(2.5) * base[0], base[1][::-1].copy(), -base[2], base[0] + base[2], np.sqrt(np.abs(base[1]))]
    assert len(fields) == abi.ADVECT_MAX_CELL_FIELDS
    car, dt = cases.carrier(grid, "random")
    s = uploaded(grid)
    try:
        rc, together, _ = s.advect(dt, fields, order=2, carrier=car)
        assert rc == abi.SUCCESS, s.last_error()
        n8 = s.array("advectionCounts")
        for q, f in enumerate(fields):
            rc, one, _ = s.advect(dt, [f], order=2, carrier=car)
            assert rc == abi.SUCCESS and one[0].tobytes() == together[q].tobytes(), q
            assert np.array_equal(s.array("advectionCounts"), n8)                  # a cell is counted once, whatever the number of fields
        want = ref.advect(cases.GRIDS[grid], float(cases.scene(grid)[0].dx), dt, 2, car, fields, False)
        assert_same((together, None, n8, float(s.array("advectionStep")[0])), want, "eight fields")
    finally:
        s.close()


def test_velocity_alone_and_cell_fields_alone():
    grid = "odd"
    car, dt = cases.carrier(grid, "random")
    fields = cases.cell_fields(grid)
    both = cases.reference(grid, "random", 2)
    s = uploaded(grid)
    try:
        rc, cout, vout = s.advect(dt, (), order=2, carrier=car, velocity=True)
        assert rc == abi.SUCCESS and cout == [], s.last_error()
        n = both[2].copy()
        n[0] = 0
        n[4] = ref.advect(cases.GRIDS[grid], float(cases.scene(grid)[0].dx), dt, 2, car, (), True)[2][4]
        assert_same(([], vout) + counts_and_step(s), ([], both[1], n, both[3]), "velocity alone")
        rc, cout, vout = s.advect(dt, fields, order=2, carrier=car, velocity=False)
        assert rc == abi.SUCCESS and vout is None, s.last_error()
        n = np.zeros(5, np.int32)
        n[0] = both[2][0]
        assert_same((cout, None) + counts_and_step(s), (both[0], None, n, both[3]), "cell fields alone")
    finally:
        s.close()


def test_two_calls_on_one_context_give_identical_bytes():
    grid = "blob"
    s = uploaded(grid)
    try:
        first = cases.run_host(s, grid, "random", 2)
        second = cases.run_host(s, grid, "random", 2)
        assert cases.digest(*first) == cases.digest(*second) == cases.digest(*cases.reference(grid, "random", 2))
    finally:
        s.close()


# ---- 2. the call changes nothing --------------------------------------------------------------------------------------------------------
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
                rc, cout, vout = s.advect(3.0 * float(sc.dt), cases.cell_fields(grid), order=2, velocity=True)
                assert rc == abi.SUCCESS, s.last_error()
                assert s.array("advectionCounts")[:4].sum() > 0
            rc = s.step_device()
            s.download()
            outcomes.append((int(rc), int(s.stats.solveData[1]), [v.tobytes() for v in s.vel], [v.tobytes() for v in s.valid], s.array("solutionVector").tobytes()))
            if call:
                assert int(s.array("advection")[0]) == 2                           # a step keeps the arrays
        finally:
            s.close()
    assert outcomes[0][1] > 0 and outcomes[0] == outcomes[1]


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing():
    grid = "odd"
    sc, p = cases.scene(grid)
    car, dt = cases.carrier(grid, "random")
    fields = cases.cell_fields(grid)
    s = polystokes_amd.Solver(0)
    try:
        d = OnDevice(grid, car, fields, abi.LAYOUT_X_FASTEST)
        host_out = [np.full(f.shape, SENTINEL, np.float32) for f in fields]
        host_vel = [np.full(c.shape, SENTINEL, np.float32) for c in car]

        def refused(why, rc=abi.INVALID, **kw):
            """the same refusal from both forms, nothing written"""
            args = dict(dt=dt, order=2, cell_in=fields, cell_out=host_out, carrier=car, vel_out=host_vel)
            dargs = dict(dt=dt, order=2, cell_in=d.cin, cell_out=d.cout, carrier=d.car, vel_out=d.vout)
            count = kw.pop("cellFields", None)
            for k, (hv, dv) in kw.items():
                args[k], dargs[k] = hv, dv
            for form, a in (("host", args), ("device", dargs)):
                A = s.advection(**a)
                if count is not None:
                    A.cellFields = count
                got = s.L.ps_advect_fields(s.h, ctypes.byref(A)) if form == "host" else s.L.ps_advect_fields_device(s.h, ctypes.byref(A), 0, None)
                assert got == rc, (form, why, got, s.last_error())
                assert why in s.last_error() and "PS_" not in s.last_error(), (form, why, s.last_error())
            assert d.untouched() and all((o == SENTINEL).all() for o in host_out + host_vel), why

        refused("call ps_upload_fields first")
        s.upload(sc, p)
        assert s.L.ps_advect_fields(s.h, None) == abi.INVALID and "a is null" in s.last_error()
        assert s.L.ps_advect_fields_device(s.h, None, 0, None) == abi.INVALID and "a is null" in s.last_error()
        for bad in (0, 3, -1):
            refused("order outside 1..2", order=(bad, bad))
        for bad in (-1, 9):
            refused("cellFields outside 0..8", cellFields=bad)
        for bad in (np.nan, np.inf, -np.inf):
            refused("dt not finite", dt=(bad, bad))
        A = s.advection(dt, 2, fields, host_out, car, host_vel)
        A.cellIn[1] = None
        assert s.L.ps_advect_fields(s.h, ctypes.byref(A)) == abi.INVALID and "cellIn[1] is null" in s.last_error()
        A = s.advection(dt, 2, d.cin, d.cout, d.car, d.vout)
        A.cellOut[2] = None
        assert s.L.ps_advect_fields_device(s.h, ctypes.byref(A), 0, None) == abi.INVALID and "cellOut[2] is null" in s.last_error()
        for holes in ((1,), (0, 2)):
            A, B = s.advection(dt, 2, fields, host_out, car, host_vel), s.advection(dt, 2, d.cin, d.cout, d.car, d.vout)
            for m in holes:
                A.carrier[m] = None
                B.velOut[m] = None
            assert s.L.ps_advect_fields(s.h, ctypes.byref(A)) == abi.INVALID and "carrier partly null" in s.last_error()
            assert s.L.ps_advect_fields_device(s.h, ctypes.byref(B), 0, None) == abi.INVALID and "velOut partly null" in s.last_error()
        refused("nothing to do", cell_in=((), ()), cell_out=((), ()), vel_out=(None, None))
        # the device form's own refusals: the layout and the pointers
        A = s.advection(dt, 2, d.cin, d.cout, d.car, d.vout)
        assert s.L.ps_advect_fields_device(s.h, ctypes.byref(A), 2, None) == abi.INVALID and "layout must be 0" in s.last_error()
        short = _hip.DeviceBuffer(d.cout[0].count - 1)
        odd = _hip.DeviceBuffer(d.cout[0].count + 1)
        for k, ptr, why in (("cellOut", host_out[0].ctypes.data, "cellOut: the pointer is not device memory"), ("cellOut", short.ptr, "cellOut: the allocation ends before"),
                            ("cellIn", odd.ptr + 2, "cellIn: the pointer is not 4-byte aligned"), ("carrier", fields[0].ctypes.data, "carrier: the pointer is not device memory"),
                            ("velOut", short.ptr, "velOut: the allocation ends before")):
            A = s.advection(dt, 2, d.cin, d.cout, d.car, d.vout)
            getattr(A, k)[0] = ptr
            assert s.L.ps_advect_fields_device(s.h, ctypes.byref(A), 0, None) == abi.INVALID, why
            assert why in s.last_error(), (why, s.last_error())
        assert d.untouched() and all((o == SENTINEL).all() for o in host_out + host_vel)
        with pytest.raises(KeyError):
            s.array("advectionCounts")                                             # no refused call registered anything
        # PS_FAILED: a null carrier before any step; the context stays usable
        A = s.advection(dt, 2, d.cin, d.cout, None, d.vout)
        assert s.L.ps_advect_fields_device(s.h, ctypes.byref(A), 0, None) == abi.FAILED and "no written velocity since the upload" in s.last_error()
        A = s.advection(dt, 2, fields, host_out, None, None)
        assert s.L.ps_advect_fields(s.h, ctypes.byref(A)) == abi.FAILED and "no written velocity since the upload" in s.last_error()
        assert d.untouched() and all((o == SENTINEL).all() for o in host_out + host_vel)
        assert s.advect_device(dt, d.cin, d.cout, order=2, carrier=d.car, vel_out=d.vout) == abi.SUCCESS, s.last_error()
        assert_same(d.outputs() + counts_and_step(s), cases.reference(grid, "random", 2), "after the refusals")
        short.close()
        odd.close()
        d.close()
    finally:
        s.close()


def test_overlapping_arrays_are_refused():
    """views of one allocation in the device form; the host form refuses host ranges the same way"""
    grid = "odd"
    car, dt = cases.carrier(grid, "random")
    fields = cases.cell_fields(grid)
    nc = fields[0].size
    nf = [c.size for c in car]
    s = uploaded(grid)
    try:
        d = OnDevice(grid, car, fields, abi.LAYOUT_X_FASTEST)
        pool = _hip.DeviceBuffer.from_numpy(np.full(4 * nc + sum(nf) + 64, SENTINEL, np.float32))
        at = lambda floats: pool.ptr + 4 * floats

        def refused(why, **kw):
            a = dict(dt=dt, order=1, cell_in=d.cin, cell_out=d.cout, carrier=d.car, vel_out=d.vout)
            a.update(kw)
            assert s.advect_device(**a) == abi.INVALID, why
            assert why in s.last_error(), (why, s.last_error())
            assert d.untouched() and (pool.to_numpy() == SENTINEL).all(), why

        refused("output 0 overlaps input 3", cell_in=[at(0)] + d.cin[1:], cell_out=[at(0)] + d.cout[1:])                    # in place
        refused("output 1 overlaps input 3", cell_in=[at(0)] + d.cin[1:], cell_out=[d.cout[0], at(nc - 1), d.cout[2]])        # by one float
        refused("output 2 overlaps output 0", cell_out=[at(8), d.cout[1], at(0)])
        refused("output 8 overlaps input 0", carrier=[at(0), d.car[1], d.car[2]], vel_out=[at(nf[0] - 1), d.vout[1], d.vout[2]])
        refused("output 9 overlaps output 8", vel_out=[at(0), at(nf[0] - 1), d.vout[2]])
        refused("output 10 overlaps input 4", cell_in=[d.cin[0], at(nf[2]), d.cin[2]], vel_out=[d.vout[0], d.vout[1], at(1)])
        # ranges that only touch are taken
        ok = dict(dt=dt, order=2, cell_in=d.cin, cell_out=[at(0), at(nc), at(2 * nc)], carrier=d.car, vel_out=d.vout)
        assert s.advect_device(**ok) == abi.SUCCESS, s.last_error()
        got = pool.to_numpy()
        want = cases.reference(grid, "random", 2)
        for q in range(3):
            assert got[q * nc:(q + 1) * nc].tobytes() == want[0][q].tobytes(), q
        assert (got[3 * nc:] == SENTINEL).all()
        # the host form
        buf = np.full(2 * nc, SENTINEL, np.float32)
        A = s.advection(dt, 1, [buf[:nc]], [buf[nc - 1:2 * nc - 1]], car, None)
        assert s.L.ps_advect_fields(s.h, ctypes.byref(A)) == abi.INVALID and "output 0 overlaps input 3" in s.last_error()
        assert (buf == SENTINEL).all()
        pool.close()
        d.close()
    finally:
        s.close()


def test_a_rank_of_a_group_is_refused():
    grid = "odd"
    sc, p = cases.scene(grid)
    car, dt = cases.carrier(grid, "random")
    g = polystokes_amd.Group(2)
    try:
        r = g.ranks[0]
        r.upload(sc, p)
        with pytest.raises(polystokes_amd.PolyStokesError, match="advection needs a single domain"):
            r.advect(dt, cases.cell_fields(grid), order=1, carrier=car)
    finally:
        g.close()


# ---- 4. memory -------------------------------------------------------------------------------------------------------------------------------
def test_memory_is_flat_and_the_counters_go_with_the_next_upload():
    grid = "blob"
    sc, p = cases.scene(grid)
    car, dt = cases.carrier(grid, "random")
    fields = cases.cell_fields(grid)
    s = uploaded(grid)
    try:
        base = s.memory_stats()["live_bytes"]
        d = OnDevice(grid, car, fields, abi.LAYOUT_X_FASTEST)                      # (the harness's own allocations are not the library's)
        seen = []
        for call in range(4):
            if call % 2:
                assert s.advect_device(dt, d.cin, d.cout, order=2, carrier=d.car, vel_out=d.vout) == abi.SUCCESS, s.last_error()
                _hip.rt().hipStreamSynchronize(None)
            else:
                cases.run_host(s, grid, "random", 2)
            mem = s.memory_stats()
            assert mem["deferred_bytes"] == 0
            seen.append(mem["live_bytes"])
        assert seen == [base + 20] * 4, (base, seen)                               # the five counters, nothing else
        s.upload(sc, p)
        mem = s.memory_stats()
        assert mem["live_bytes"] == base and mem["deferred_bytes"] == 0, (base, mem)
        for name in ("advection", "advectionStep", "advectionCounts"):
            with pytest.raises(KeyError):
                s.array(name)
        d.close()
    finally:
        s.close()


# ---- 5. other builds and switches, each in a process of its own ---------------------------------------------------------------------------
CHILD_CASES = ("blob:random:2", "odd:nonfinite:1", "odd:random:2", "blob:shift:1")


def _child(env, expect=()):
    pr = children.run_script("advection_cases.py", "advect", *CHILD_CASES, limit=300, env=env, drop=() if "PS_LIB" in env else ("PS_LIB",), expect=expect)
    want = {}
    for name in CHILD_CASES:
        grid, kind, order = name.split(":")
        want[name] = cases.digest(*cases.reference(grid, kind, int(order)))
    assert dict(pr.digests()) == want, pr.output[-2000:]


def test_poisoned_buffers_change_nothing():
    """PS_DEBUG_POISON=1 fills whatever a buffer allocation hands out with 0xff: a kernel that read a word nobody wrote would show"""
    _child({"PS_DEBUG_POISON": "1"}, expect=["PS_DEBUG_POISON=1 is active"])


def test_the_release_library_gives_the_same_bytes():
    _child({"PS_LIB": RELEASE})

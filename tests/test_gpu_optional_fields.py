"""The four optional cell fields (density, free-surface sigma / pressure, contact cosine, collider ids) through one lifecycle: each entry
point, from a host array and from a device array in either layout, on a 70 x 5 x 9 grid (x passes the 64-wide tile of the transposition,
3150 cells leave the 16-byte copy a scalar tail).  Only uploads, setups and small steps: every figure below is what the library did before
the upload paths were folded into one, and pins it: error strings, the x-fastest index of a refused value, live_bytes to the byte.

Two things the density field does differently, and keeps doing: its buffer stays with the context once allocated (None and a fresh upload
switch the field off without freeing it), and a device upload keeps the 12 bytes of scan words it allocated."""
import numpy as np
import pytest

import polystokes_amd
from polystokes_amd import _abi as abi
from polystokes_amd import _hip, scenes

pytestmark = pytest.mark.gpu

NX, NY, NZ = 70, 5, 9
CELLS = NX * NY * NZ
SCAN_BYTES = 12                                      # the three words of the field scan
# two cells, A < B in x-fastest numbering, in different 64-tiles of x and different z-planes; B comes first in z-fastest storage
KA, JA, IA = 2, 3, 66
KB, JB, IB = 6, 1, 3
A = IA + NX * (JA + NY * KA)
B = IB + NX * (JB + NY * KB)
assert A < B and IA // 64 != IB // 64 and KB + NZ * (JB + NY * IB) < KA + NZ * (JA + NY * IA)

FIELDS = ("density", "surface", "contact", "ids")
SOURCES = ("host", "device0", "device1")
HOST_NAME = {"density": "ps_upload_density_field", "surface": "ps_upload_surface_fields", "contact": "ps_upload_contact_cosine_field",
             "ids": "ps_upload_collider_ids"}
LABEL = {"density": "density", "surface": "sigma", "contact": "cosTheta", "ids": "ids"}       # of the first pointer in a refusal


@pytest.fixture(scope="module")
def scene():
    sc, p = scenes.blob(NX, NY, NZ, seed=3)
    sc.surface_tension = 0.5                         # the curvature runs, so a cosine field switches the contact rule on
    return sc, p


def _good(field):
    """the arrays of one call (two for the surface fields), shape (z, y, x)"""
    rng = np.random.RandomState(7)
    sh = (NZ, NY, NX)
    if field == "density":
        return ((900.0 * (1.0 + rng.uniform(0, 1, sh))).astype(np.float32),)
    if field == "surface":
        return rng.uniform(0.1, 1.0, sh).astype(np.float32), rng.uniform(-5, 5, sh).astype(np.float32)
    if field == "contact":
        return (rng.uniform(-1, 1, sh).astype(np.float32),)
    return (rng.randint(0, 3, sh).astype(np.int32),)


def _bad(field):
    """[(arrays with two bad values, the refusal after the host function's name)]"""
    def plant(a, va, vb):
        a = a.copy()
        a[KA, JA, IA], a[KB, JB, IB] = va, vb
        return a
    g = _good(field)
    if field == "density":
        return [((plant(g[0], np.nan, np.inf),), "non-finite value at cell %d" % A)]
    if field == "surface":
        return [((plant(g[0], -1.0, np.nan), g[1]), "sigma: non-finite or negative value at cell %d" % A),
                ((g[0], plant(g[1], np.inf, np.nan)), "pressure: non-finite value at cell %d" % A),
                ((None, plant(g[1], -np.inf, np.inf)), "pressure: non-finite value at cell %d" % A)]
    if field == "contact":
        return [((plant(g[0], 1.5, np.nan),), "contact cosine: value outside [-1, 1] at cell %d" % A)]
    return []


class Call:
    """one field's entry point from one source; device buffers live until close()"""

    def __init__(self, s, field, source):
        self.s, self.field, self.source = s, field, source
        self.layout = None if source == "host" else int(source[-1])
        self.bufs = []

    def device(self, a, pad=0):
        if a is None:
            return None
        b = _hip.DeviceBuffer.from_numpy(polystokes_amd.to_layout(a.view(np.float32), self.layout), pad)
        self.bufs.append(b)
        return b

    def raw(self, args, layout):
        """the _device entry point on addresses"""
        s = self.s
        if self.field == "density":
            return s.upload_density_field_device(args[0], layout)
        if self.field == "surface":
            return s.upload_surface_fields_device(args[0], args[1], layout)
        if self.field == "contact":
            return s.upload_contact_cosine_field_device(args[0], layout)
        return s.upload_collider_ids_device(args[0], layout)

    def host(self, arrays):
        s = self.s
        if self.field == "density":
            return s.upload_density_field(arrays[0])
        if self.field == "surface":
            return s.upload_surface_fields(arrays[0], arrays[1])
        if self.field == "contact":
            return s.upload_contact_cosine_field(arrays[0])
        return s.upload_collider_ids(arrays[0])

    def __call__(self, arrays):
        """arrays: what _good / _bad return, or None to drop the field"""
        if arrays is None:
            arrays = (None, None)
        if self.source == "host":
            return self.host(arrays)
        return self.raw([self.device(a, pad=1) for a in arrays], self.layout)      # (pointers that are only 4-byte aligned)

    def close(self):
        for b in self.bufs:
            b.close()
        self.bufs = []


def _used(s, field):
    """after a setup: did it use the field?  (ids: no status array; their presence is read from live_bytes)"""
    if field == "density":
        return int(s.array("densityField")[0]) == 1
    if field == "surface":
        return int(s.array("surfaceFields")[0]) != 0
    try:
        return int(s.array("contactField")[0]) == 1
    except KeyError:
        return False


def _mem(s):
    m = s.memory_stats()
    return m["live_bytes"], m["deferred_bytes"]


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("field", FIELDS)
def test_lifecycle(scene, field, source):
    sc, p = scene
    s = polystokes_amd.Solver(0)
    call = Call(s, field, source)
    good = _good(field)
    scan = SCAN_BYTES if source != "host" else 0
    try:
        # (a) before any upload: the host function's name, from either entry point
        assert call(good) == abi.INVALID
        assert s.last_error() == HOST_NAME[field] + ": call ps_upload_fields first", s.last_error()
        s.upload(sc, p)
        assert s.setup() == abi.SUCCESS
        assert not _used(s, field)
        base, deferred = _mem(s)
        assert deferred == 0

        # (b) a good field is used by the next setup
        assert call(good) == abi.SUCCESS, s.last_error()
        live, deferred = _mem(s)
        print(field, source, "good field: live_bytes +", live - base)
        present = 4 * CELLS * len(good) + (scan if field == "density" else 0)       # (every other call frees the scan words it allocated)
        assert (live - base, deferred) == (present, 0)
        assert s.setup() == abi.SUCCESS
        if field != "ids":
            assert _used(s, field)

        # (c) two bad values: the x-fastest index of the first, the host call's message character for character
        for arrays, why in _bad(field):
            assert call(good) == abi.SUCCESS
            assert call.host(arrays) == abi.INVALID
            host_message = s.last_error()
            assert host_message == HOST_NAME[field] + ": " + why, host_message
            assert call(good) == abi.SUCCESS
            assert call(arrays) == abi.INVALID
            assert s.last_error() == host_message, (s.last_error(), host_message)
            # (d) a refused value leaves the field dropped
            assert _mem(s)[1] == 0
            assert s.setup() == abi.SUCCESS
            assert not _used(s, field)
            assert _mem(s)[1] == 0

        # (e) None drops the field and its bytes (the density buffer stays)
        assert call(None) == abi.SUCCESS
        assert s.setup() == abi.SUCCESS                       # (buffers a setup holds only while the field is present go here)
        before = _mem(s)[0]
        assert call(good) == abi.SUCCESS
        assert call(None) == abi.SUCCESS
        live, deferred = _mem(s)
        print(field, source, "None: live_bytes +", live - before)
        assert (live - before, deferred) == (0, 0)
        assert s.setup() == abi.SUCCESS
        assert not _used(s, field)

        # (g) the pointer and layout refusals of the _device entry point carry its name and change nothing, except that the surface
        # fields are dropped; the context still steps
        if source != "host":
            dev_name = HOST_NAME[field] + "_device"
            ok = [call.device(a, pad=1) for a in good]
            host_array = np.zeros(CELLS, np.float32)
            rest = ok[1:]
            for first, layout, why in (
                    (ok[0].ptr + 2, call.layout, LABEL[field] + ": the pointer is not 4-byte aligned"),
                    (host_array.ctypes.data, call.layout, LABEL[field] + ": the pointer is not device memory of the context's device"),
                    (ok[0].ptr + 8, call.layout, LABEL[field] + ": the allocation ends before the field does (%d floats needed)" % CELLS),
                    (ok[0], 2, "layout must be 0 (x fastest) or 1 (z fastest)")):
                assert call.raw(ok, call.layout) == abi.SUCCESS, s.last_error()
                held = _mem(s)[0]
                assert call.raw([first] + rest, layout) == abi.INVALID, why
                assert s.last_error() == dev_name + ": " + why, s.last_error()
                live, deferred = _mem(s)
                assert deferred == 0
                assert held - live == (4 * CELLS * len(good) if field == "surface" else 0), (field, why)
                assert s.step_device() == abi.SUCCESS, why
                if field != "ids":
                    assert _used(s, field) == (field != "surface"), why
            assert call(None) == abi.SUCCESS

        # (f) a fresh ps_upload_fields drops all four, released at once: the bytes of a context that never had them
        assert s.setup() == abi.SUCCESS
        never = _mem(s)[0]
        others = [Call(s, f, source) for f in FIELDS]
        for c in others:
            assert c(_good(c.field)) == abi.SUCCESS, (c.field, s.last_error())
        full = _mem(s)[0]
        # what a density field leaves behind for good: its buffer and, from a device source, the scan words (this case's own field
        # allocated them long ago when it is the density)
        residue = 0 if field == "density" else 4 * CELLS + scan
        assert full - never == 4 * CELLS * 4 + residue, full - never
        s.upload(sc, p)
        live, deferred = _mem(s)
        print(field, source, "fresh upload: live_bytes +", live - never)
        assert (live - never, deferred) == (residue, 0)
        assert s.setup() == abi.SUCCESS
        assert not any(_used(s, f) for f in ("density", "surface", "contact"))
        assert _mem(s) == (never + residue, 0)
        for c in others:
            c.close()
    finally:
        call.close()
        s.close()

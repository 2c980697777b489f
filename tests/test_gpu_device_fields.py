"""Device-resident fields (ps_*_device) on the GPU: the same values through GPU pointers in either axis order must leave the context and
the outputs exactly as the host entry points do.  Every comparison is on the bytes: the device path fills the same buffers with the same
values, and the step is deterministic (the first test is that control)."""
import os
import sys

import numpy as np
import pytest

import polystokes_amd
from polystokes_amd import _abi as abi, scenes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import children  # noqa: E402
import device_fields_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = (abi.LAYOUT_X_FASTEST, abi.LAYOUT_Z_FASTEST)
_ref = {}


def _scene(name):
    return cases.weights_scene() if name == "blob_weights" else cases.scene(name)


def host_reference(name):
    """One host-boundary step of scene `name` on a fresh context, computed once and shared (never modified)."""
    if name not in _ref:
        sc, p = _scene(name)
        s = polystokes_amd.Solver(0)
        _ref[name] = (sc, p, cases.host_step(s, sc, p))
        s.close()
    return _ref[name]


SCENES = ("blob", "blob_uniform", "cavity32", "blob_weights")


@pytest.mark.parametrize("name", SCENES)
def test_control_two_host_contexts_agree_bit_for_bit(name):
    sc, p, ref = host_reference(name)
    s = polystokes_amd.Solver(0)
    again = cases.host_step(s, sc, p)
    s.close()
    assert not cases.same(ref, again)
    assert int(ref["rc"]) in (abi.SUCCESS, abi.NOCONVERGE)


# ---- 1. the kernels alone ------------------------------------------------------------------------------------------------------
def _passthrough(dims, lin, lout, pad=0):
    """doSolve = 0 and keepNonConvergedResults = 0: the step copies vel to the output on every face, so upload in one layout and download
    in another must return the input, re-laid-out by numpy."""
    sc, p = scenes.blob(*dims)
    p.doSolve, p.keepNonConvergedResults = 0, 0
    s = polystokes_amd.Solver(0)
    ds = polystokes_amd.device_scene(sc, lin, pad)
    assert s.upload_device(p, ds, lin) == abi.SUCCESS, s.last_error()
    s.step_device()
    rc, vel, valid = s.download_device(lout)
    assert rc == abi.SUCCESS, s.last_error()
    got, _ = cases.device_outputs(sc, vel, valid, lout)
    for a in range(3):
        assert got[a].tobytes() == sc.vel[a].tobytes(), (dims, lin, lout, a)
        # and the flat device order is the numpy re-layout of the host array
        assert vel[a].to_numpy().tobytes() == polystokes_amd.to_layout(sc.vel[a], lout).tobytes()
    s.close()


# (24, 20, 28): every extent below one 64-tile; (64, 9, 63): extents 63, 64 and 65 over the cell and face grids; (70, 12, 66): more than
# one tile with a remainder along both swapped axes
@pytest.mark.parametrize("dims", [(24, 20, 28), (64, 9, 63), (70, 12, 66)])
@pytest.mark.parametrize("lin", LAYOUTS)
@pytest.mark.parametrize("lout", LAYOUTS)
def test_layouts_round_trip_through_the_kernels(dims, lin, lout):
    _passthrough(dims, lin, lout)


@pytest.mark.parametrize("lin", LAYOUTS)
def test_pointers_offset_by_one_float_take_the_scalar_copy(lin):
    """every input one float into a larger allocation: 4-byte aligned only (a view with a storage offset)"""
    _passthrough((70, 12, 66), lin, abi.LAYOUT_X_FASTEST, pad=1)


# ---- 2. whole step, every input field ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_step_through_device_fields_equals_the_host_step(name, layout):
    sc, p, ref = host_reference(name)
    s = polystokes_amd.Solver(0)
    got = cases.device_step(s, sc, p, layout)
    s.close()
    assert not cases.same(ref, got)


# ---- 3. density field ----------------------------------------------------------------------------------------------------------
def _density_step(s, sc, p, layout=None):
    """upload, density field, step, download — host calls (layout None) or device calls"""
    if layout is None:
        s.upload(sc, p)
        rc = s.step_device()
        s.download()
        return cases.collect(s, rc, s.vel, s.valid), int(s.array("densityField")[0])
    ds = polystokes_amd.device_scene(sc, layout)
    assert s.upload_device(p, ds, layout) == abi.SUCCESS, s.last_error()
    assert s.upload_density_field_device(ds.density_field, layout) == abi.SUCCESS, s.last_error()
    rc = s.step_device()
    _, vel, valid = s.download_device(layout)
    v, ok = cases.device_outputs(sc, vel, valid, layout)
    return cases.collect(s, rc, v, ok), int(s.array("densityField")[0])


@pytest.mark.parametrize("kind", ["smooth", "constant"])
def test_density_field_from_the_device(kind):
    sc, p = cases.scene("blob")
    if kind == "smooth":
        scenes.with_density_field(sc, "smooth")
    else:
        sc.density_field = np.full((sc.nz, sc.ny, sc.nx), 450.0, np.float32)
    s = polystokes_amd.Solver(0)
    ref, used = _density_step(s, sc, p)
    s.close()
    assert used == (1 if kind == "smooth" else 0)
    for layout in LAYOUTS:
        s = polystokes_amd.Solver(0)
        got, used_dev = _density_step(s, sc, p, layout)
        s.close()
        assert used_dev == used, layout
        assert not cases.same(ref, got), layout


def test_density_field_with_a_nan_is_refused_with_the_host_index():
    sc, p, ref = host_reference("blob")
    rho = np.full((sc.nz, sc.ny, sc.nx), 450.0, np.float32)
    rho[5, 3, 7] = np.nan
    rho[9, 1, 2] = np.inf                          # a later one in x-fastest order, an earlier one in z-fastest order
    s = polystokes_amd.Solver(0)
    s.upload(sc, p)
    assert s.upload_density_field(rho) == abi.INVALID
    want = s.last_error()
    assert want.endswith("non-finite value at cell %d" % (7 + sc.nx * (3 + sc.ny * 5))), want
    from polystokes_amd import _hip
    for layout in LAYOUTS:
        ds = polystokes_amd.device_scene(sc, layout)
        assert s.upload_device(p, ds, layout) == abi.SUCCESS
        d = _hip.DeviceBuffer.from_numpy(polystokes_amd.to_layout(rho, layout))
        assert s.upload_density_field_device(d, layout) == abi.INVALID
        assert s.last_error() == want
        rc = s.step_device()                        # the field is dropped: the step is the scalar one
        _, vel, valid = s.download_device(layout)
        v, ok = cases.device_outputs(sc, vel, valid, layout)
        assert not cases.same(ref, cases.collect(s, rc, v, ok)), layout
    s.close()


# ---- 4. solution fields --------------------------------------------------------------------------------------------------------
def test_solution_fields_on_the_device_equal_the_host_download():
    sc, p, _ = host_reference("blob")
    s = polystokes_amd.Solver(0)
    s.step(sc, p)
    want = s.solution_fields()
    assert any(np.any(v != 0) for v in want.values())
    for layout in LAYOUTS:
        got = s.solution_fields_device(layout)
        for name, grid in abi.SOLUTION_FIELDS:
            back = polystokes_amd.from_layout(got[name].to_numpy(), want[name].shape, layout)
            assert back.tobytes() == want[name].tobytes(), (layout, name)
    s.close()


# ---- 5. streams ----------------------------------------------------------------------------------------------------------------
def test_caller_stream_orders_inputs_and_outputs():
    """The inputs are filled by async copies queued on the caller's stream and never waited for by the host; the outputs are read by an
    async copy queued on it after the download; only that stream is synchronised."""
    from polystokes_amd import _hip
    sc, p, ref = host_reference("blob")
    layout = abi.LAYOUT_Z_FASTEST
    staging = polystokes_amd.device_scene(sc, layout)
    live = polystokes_amd.device_scene(sc, layout)
    st = _hip.Stream()
    pairs = list(zip(live.vel + live.collisionvel + [live.surface, live.collision, live.viscosity],
                     staging.vel + staging.collisionvel + [staging.surface, staging.collision, staging.viscosity]))
    junk = np.full(max(b.count for b, _ in pairs), 7.5, np.float32)
    for dst, _ in pairs:                                            # what the step would see if it did not wait for the stream
        _hip.memcpy(dst.ptr, junk.ctypes.data, dst.nbytes, _hip.H2D)
    s = polystokes_amd.Solver(0)
    for dst, src in pairs:
        _hip.memcpy_async(dst.ptr, src.ptr, dst.nbytes, _hip.D2D, st.cuda_stream)
    assert s.upload_device(p, live, layout, stream=st) == abi.SUCCESS, s.last_error()
    rc = s.step_device()
    _, vel, valid = s.download_device(layout, stream=st)
    host = [_hip.HostBuffer(b.count) for b in vel + valid]
    for h, b in zip(host, vel + valid):
        _hip.memcpy_async(h.ptr, b.ptr, b.nbytes, _hip.D2H, st.cuda_stream)
    st.synchronize()
    sh = abi.grid_shapes(sc.nx, sc.ny, sc.nz)
    back = [polystokes_amd.from_layout(np.array(h.array), sh["face" + "XYZ"[q % 3]], layout) for q, h in enumerate(host)]
    got = cases.collect(s, rc, back[:3], back[3:])
    s.close()
    for h in host:
        h.close()
    st.close()
    assert not cases.same(ref, got)


# ---- 6. aliasing ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_output_velocity_may_alias_the_input(layout):
    sc, p, ref = host_reference("blob")
    s = polystokes_amd.Solver(0)
    got = cases.device_step(s, sc, p, layout, alias=True)
    s.close()
    assert not cases.same(ref, got)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_context_usable():
    from polystokes_amd import _hip
    sc, p, ref = host_reference("blob")
    # blob's faceX grid: 25 * 20 * 28 floats = 56000 bytes, not a multiple of 4096 (a missed length check would read inside the last page)
    assert (sc.vel[0].nbytes % 4096) != 0
    s = polystokes_amd.Solver(0)

    class Fields:
        pass

    def variant(**kw):
        ds = polystokes_amd.device_scene(sc, 0)
        f = Fields()
        f.__dict__.update(ds.__dict__)
        f.vel = list(ds.vel)
        f.__dict__.update(kw)
        f._keep = ds
        return f

    pinned = _hip.HostBuffer(sc.surface.size)
    pinned.array[:] = sc.surface.ravel()
    short = _hip.DeviceBuffer.from_numpy(sc.vel[0].ravel()[:-1])
    base = variant()
    refusals = [
        ("layout", base, 2, "layout must be 0 (x fastest) or 1 (z fastest)"),
        ("null surface", variant(surface=None), 0, "Surface field is missing."),
        ("pinned host", variant(surface=pinned.ptr), 0, "not device memory of the context's device"),
        ("misaligned", variant(viscosity=base.viscosity.ptr + 2), 0, "not 4-byte aligned"),
        ("short", variant(vel=[short, base.vel[1], base.vel[2]]), 0, "the allocation ends before the field does"),
    ]
    for what, f, layout, message in refusals:
        assert s.upload_device(p, f, layout) == abi.INVALID, what
        assert message in s.last_error(), (what, s.last_error())
        rc, _, _ = s.step_device_fields(p, f, layout)
        assert rc == abi.INVALID and message in s.last_error(), (what, s.last_error())
        got = cases.device_step(s, sc, p, abi.LAYOUT_Z_FASTEST)          # the next step runs, and correctly
        assert not cases.same(ref, got), what
    # an output that is too short is refused before the step runs
    out = ([short, _hip.DeviceBuffer(sc.vel[1].size), _hip.DeviceBuffer(sc.vel[2].size)], [None, None, None])
    rc, _, _ = s.step_device_fields(p, base, 0, out=out)
    assert rc == abi.INVALID and "the allocation ends before the field does" in s.last_error()
    s.close()
    pinned.close()


# ---- 8. reuse ------------------------------------------------------------------------------------------------------------------
def test_alternating_host_and_device_uploads_do_not_grow_the_context():
    sc, p, ref = host_reference("blob")
    s = polystokes_amd.Solver(0)
    live = []
    for step in range(5):
        got = cases.host_step(s, sc, p) if step % 2 == 0 else cases.device_step(s, sc, p, abi.LAYOUT_Z_FASTEST)
        assert not cases.same(ref, got), step
        m = s.memory_stats()
        assert m["deferred_bytes"] == 0, step
        live.append(m["live_bytes"])
    s.close()
    assert len(set(live[1:])) == 1, live


# ---- 9. decomposition ----------------------------------------------------------------------------------------------------------
def test_group_ranks_take_the_device_upload():
    from polystokes_amd import partition
    sc, p = scenes.cavity(32)
    g = polystokes_amd.Group(2)
    rc_host = g.solve_scene(sc, p)
    want = [v.copy() for v in g.vel]
    g.close()
    for layout in LAYOUTS:
        g = polystokes_amd.Group(2)
        slabs = [partition.make_slab(sc.nz, 2, r, p.tileSize) for r in range(2)]
        for r, sl in enumerate(slabs):
            local = partition.local_scene(sc, sl)
            assert g.ranks[r].upload_device(p, polystokes_amd.device_scene(local, layout), layout) == abi.SUCCESS
            g.ranks[r].set_slab(sl)
        assert g.step() == rc_host
        vel = [np.array(sc.vel[a], copy=True) for a in range(3)]
        for r, sl in enumerate(slabs):
            lv, _ = g.ranks[r].download()
            for a in range(3):
                partition.merge_faces(vel[a], lv[a], g.ranks[r].array("owned" + "XYZ"[a]), sl, a)
        g.close()
        for a in range(3):
            assert vel[a].tobytes() == want[a].tobytes(), (layout, a)


# ---- 10. torch, and the release library ----------------------------------------------------------------------------------------
def _child(mode, env_extra):
    return children.run_script("device_fields_cases.py", mode, limit=600, env=env_extra, drop=("PS_LIB",)).output


def test_torch_tensors_on_the_current_stream():
    out = _child("torch", {})
    if "CHILD SKIP" in out:
        pytest.skip("torch.cuda.is_available() is false")
    assert "CHILD OK" in out, out[-2000:]


def test_release_library_steps_through_device_fields():
    rel = os.path.join(ROOT, "polystokes_amd", "libpolystokes_hip_release.so")
    assert os.path.exists(rel), "build it: make -C polystokes_amd/csrc"
    assert "CHILD OK" in _child("release", {"PS_LIB": rel})

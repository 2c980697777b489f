"""Contact angles (ps_set_contact_angle, ps_upload_contact_cosine_field) without a GPU: the declarations and exports in both libraries,
the argtypes, the documented names, the Scene attributes, the decompositions' cuts of the cosine field, and the Houdini shim's row."""
import ctypes
import os
import re

import numpy as np
import pytest

from polystokes_amd import _abi as abi
from polystokes_amd import partition, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ps_set_contact_angle", "ps_upload_contact_cosine_field", "ps_upload_contact_cosine_field_device"]


def test_header_declares_the_entry_points_the_constant_and_the_arrays():
    hdr = open(os.path.join(ROOT, "include", "polystokes.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"#define\s+PS_CONTACT_ANGLE_SWEEPS\s+6\b", code)
    assert abi.CONTACT_ANGLE_SWEEPS == 6
    assert re.search(r"int32_t\s+ps_set_contact_angle\s*\(\s*ps_context\s*\*\s*ctx\s*,\s*double\s+degrees\s*\)\s*;", code)
    assert re.search(r"int32_t\s+ps_upload_contact_cosine_field\s*\(\s*ps_context\s*\*\s*ctx\s*,\s*const\s+float\s*\*\s*cosTheta\s*\)\s*;", code)
    assert re.search(r"int32_t\s+ps_upload_contact_cosine_field_device\s*\(\s*ps_context\s*\*\s*ctx\s*,\s*const\s+float\s*\*\s*cosTheta\s*,"
                     r"\s*int32_t\s+layout\s*,\s*void\s*\*\s*stream\s*\)\s*;", code)
    for name in ('"contactAngle"', '"contactCosine"', '"contactField"', '"contactCells"', '"surfaceWetted"',
                 "contact angle outside 0..180", "contact cosine: value outside [-1, 1] at cell N"):
        assert name in hdr, name
    assert "there are no contact angles" not in re.sub(r"\s+\*\s+", " ", hdr)           # the free-surface paragraph points to the call now
    for word in ("contact angles", "hysteresis", "two fp32 cell grids"):                 # what it costs and leaves out is said
        assert word in hdr, word


def test_both_libraries_export_them_and_the_argtypes_are_set():
    import polystokes_amd
    L = polystokes_amd.lib()
    rel = ctypes.CDLL(os.path.join(ROOT, "polystokes_amd", "libpolystokes_hip_release.so"))
    aff = ctypes.CDLL(os.path.join(ROOT, "polystokes_amd", "libpolystokes_hip_affine.so"))
    for name in NAMES:
        assert name in polystokes_amd.EXPORTED_SYMBOLS
        assert hasattr(L, name) and hasattr(rel, name) and hasattr(aff, name), name
        assert getattr(L, name).restype is ctypes.c_int32
    assert L.ps_set_contact_angle.argtypes == [ctypes.c_void_p, ctypes.c_double]
    assert L.ps_upload_contact_cosine_field.argtypes == [ctypes.c_void_p, ctypes.c_void_p]
    assert L.ps_upload_contact_cosine_field_device.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    assert L.ps_abi_version() == 1
    assert L.ps_set_contact_angle(None, 60.0) == abi.FAILED                        # no context
    assert L.ps_upload_contact_cosine_field(None, None) == abi.FAILED
    assert L.ps_upload_contact_cosine_field_device(None, None, 0, None) == abi.FAILED
    for name, kind in (("contactAngle", "f"), ("contactCosine", "f"), ("contactField", "i"), ("contactCells", "i"), ("surfaceWetted", "f")):
        assert polystokes_amd._kind(name) == kind, name
    for name in ("set_contact_angle", "upload_contact_cosine_field", "upload_contact_cosine_field_device"):
        assert callable(getattr(polystokes_amd.Solver, name)), name
    assert callable(polystokes_amd.Group.set_contact_angle)


def test_scene_attributes():
    sc, p = scenes.droplet(24)
    assert sc.contact_angle is None and sc.contact_cosine_field is None
    sh = (sc.nz, sc.ny, sc.nx)
    s2 = abi.Scene(sc.nx, sc.ny, sc.nz, sc.dx, sc.dt, sc.density, sc.vel, sc.surface, sc.collision, sc.viscosity,
                   contact_angle=60, contact_cosine_field=np.arange(np.prod(sh)).reshape(sh))
    assert s2.contact_angle == 60.0 and isinstance(s2.contact_angle, float)
    assert s2.contact_cosine_field.shape == sh and s2.contact_cosine_field.dtype == np.float32 and s2.contact_cosine_field.flags["C_CONTIGUOUS"]
    assert s2.contact_cosine_field[1, 2, 3] == (1 * sc.ny + 2) * sc.nx + 3
    s3, _ = scenes.sessile_drop(16, sigma=1.0, contact_angle=120.0)
    assert s3.contact_angle == 120.0 and s3.surface_tension == 1.0 and s3.contact_cosine_field is None
    assert (s3.collision[:, :4, :] < 0).all() and (s3.collision[:, 4:, :] > 0).all()


def _field_scene(n=(24, 20, 64), tile=8):
    """the field carries every cell's linear index, so that any mis-cut shows"""
    sc, p = scenes.blob(*n, seed=3, tile=tile)
    sc.contact_cosine_field = np.arange(sc.viscosity.size, dtype=np.float32).reshape(sc.viscosity.shape) + 0.5
    sc.contact_angle = 75.0
    return sc, p


@pytest.mark.parametrize("world", [2, 3])
def test_slab_cuts_of_the_cosine_field(world):
    sc, p = _field_scene()
    for r in range(world):
        sl = partition.make_slab(sc.nz, world, r, p.tileSize)
        loc = partition.local_scene(sc, sl)
        got = loc.contact_cosine_field
        assert got is not None and got.shape == loc.viscosity.shape and got.dtype == np.float32
        assert np.array_equal(got, sc.contact_cosine_field[sl.g0:sl.g0 + sl.nz_local])
        assert loc.contact_angle == 75.0
    sc.contact_cosine_field, sc.contact_angle = None, None
    loc = partition.local_scene(sc, partition.make_slab(sc.nz, 2, 0, p.tileSize))
    assert loc.contact_cosine_field is None and loc.contact_angle is None


def test_brick_cuts_of_the_cosine_field():
    sc, p = _field_scene((32, 32, 32), tile=8)
    for r in range(8):
        b = partition.make_brick((sc.nx, sc.ny, sc.nz), (2, 2, 2), r, p.tileSize)
        loc = partition.local_scene_brick(sc, b)
        ox, oy, oz = b.origin
        nx, ny, nz = b.n_local
        assert loc.contact_cosine_field.shape == (nz, ny, nx)
        assert np.array_equal(loc.contact_cosine_field, sc.contact_cosine_field[oz:oz + nz, oy:oy + ny, ox:ox + nx])
        assert loc.contact_angle == 75.0
    sc.contact_cosine_field = None
    loc = partition.local_scene_brick(sc, partition.make_brick((sc.nx, sc.ny, sc.nz), (2, 2, 2), 0, p.tileSize))
    assert loc.contact_cosine_field is None and loc.contact_angle == 75.0


def test_shim_has_the_angle_row_off_by_default():
    src = open(os.path.join(ROOT, "shim", "HDK_PolyStokes_shim.C")).read()
    hdr = open(os.path.join(ROOT, "shim", "HDK_PolyStokes_shim.h")).read()
    m = re.search(r"\{'F',\s*\"contactAngle\",\s*\"[^\"]*\",\s*nullptr,\s*([-0-9.e]+)\}", src)
    assert m and float(m.group(1)) == -1
    assert 'GET_DATA_FUNC_F("contactAngle"' in hdr
    call = src.index("ps_set_contact_angle(myCtx, (double)getContactAngle())")
    assert call < src.index("result = polystokes_step(")                                   # passed before the step

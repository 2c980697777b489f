"""Free-surface fields (ps_upload_surface_fields) without a GPU: the declarations and exports in both libraries, the argtypes, the
documented array names, the Scene attributes, the decompositions' cuts of both fields, and the Houdini shim's two rows."""
import ctypes
import os
import re

import numpy as np
import pytest

from polystokes_amd import _abi as abi
from polystokes_amd import partition, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ps_upload_surface_fields", "ps_upload_surface_fields_device"]


def test_header_declares_the_struct_the_entry_points_and_the_arrays():
    hdr = open(os.path.join(ROOT, "include", "polystokes.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"typedef\s+struct\s+ps_surface_fields\s*\{\s*const\s+float\s*\*\s*sigma\s*;\s*const\s+float\s*\*\s*pressure\s*;\s*\}\s*ps_surface_fields\s*;", code)
    assert re.search(r"int32_t\s+ps_upload_surface_fields\s*\(\s*ps_context\s*\*\s*ctx\s*,\s*const\s+ps_surface_fields\s*\*\s*f\s*\)\s*;", code)
    assert re.search(r"int32_t\s+ps_upload_surface_fields_device\s*\(\s*ps_context\s*\*\s*ctx\s*,\s*const\s+ps_surface_fields\s*\*\s*f\s*,"
                     r"\s*int32_t\s+layout\s*,\s*void\s*\*\s*stream\s*\)\s*;", code)
    for name in ('"surfaceFields"', '"surfaceGhostPressure"', "sigma: non-finite or negative value at cell N", "pressure: non-finite value at cell N"):
        assert name in hdr, name
    for word in ("Marangoni", "contact angles", "closest interface point", "bubble model"):      # what the feature leaves out is said
        assert word in hdr, word


def test_both_libraries_export_them_and_the_argtypes_are_set():
    import polystokes_amd
    L = polystokes_amd.lib()
    rel = ctypes.CDLL(os.path.join(ROOT, "polystokes_amd", "libpolystokes_hip_release.so"))
    for name in NAMES:
        assert name in polystokes_amd.EXPORTED_SYMBOLS
        assert hasattr(L, name) and hasattr(rel, name), name
        assert getattr(L, name).restype is ctypes.c_int32
    assert L.ps_upload_surface_fields.argtypes == [ctypes.c_void_p, ctypes.POINTER(abi.SurfaceFields)]
    assert L.ps_upload_surface_fields_device.argtypes == [ctypes.c_void_p, ctypes.POINTER(abi.SurfaceFields), ctypes.c_int32, ctypes.c_void_p]
    assert [f[0] for f in abi.SurfaceFields._fields_] == ["sigma", "pressure"]
    assert ctypes.sizeof(abi.SurfaceFields) == 2 * ctypes.sizeof(ctypes.c_void_p)
    assert L.ps_abi_version() == 1
    assert L.ps_upload_surface_fields(None, None) == abi.FAILED                   # no context
    assert L.ps_upload_surface_fields_device(None, None, 0, None) == abi.FAILED
    assert polystokes_amd._kind("surfaceFields") == "i" and polystokes_amd._kind("surfaceGhostPressure") == "f"


def test_scene_attributes():
    sc, p = scenes.droplet(24)
    assert sc.surface_sigma_field is None and sc.surface_pressure_field is None
    sh = (sc.nz, sc.ny, sc.nx)
    s2 = abi.Scene(sc.nx, sc.ny, sc.nz, sc.dx, sc.dt, sc.density, sc.vel, sc.surface, sc.collision, sc.viscosity,
                   surface_sigma_field=0.5, surface_pressure_field=np.arange(np.prod(sh)).reshape(sh))
    assert s2.surface_sigma_field.shape == sh and s2.surface_sigma_field.dtype == np.float32 and (s2.surface_sigma_field == 0.5).all()
    assert s2.surface_pressure_field.dtype == np.float32 and s2.surface_pressure_field.flags["C_CONTIGUOUS"]
    assert s2.surface_pressure_field[1, 2, 3] == (1 * sc.ny + 2) * sc.nx + 3


def _field_scene(n=(24, 20, 64), tile=8):
    """both fields carry every cell's linear index (with different offsets), so that any mis-cut shows"""
    sc, p = scenes.blob(*n, seed=3, tile=tile)
    idx = np.arange(sc.viscosity.size, dtype=np.float32).reshape(sc.viscosity.shape)
    sc.surface_sigma_field = idx + 0.5
    sc.surface_pressure_field = -idx - 1.0
    return sc, p


@pytest.mark.parametrize("world", [2, 3])
def test_slab_cuts_of_both_fields(world):
    sc, p = _field_scene()
    for r in range(world):
        sl = partition.make_slab(sc.nz, world, r, p.tileSize)
        loc = partition.local_scene(sc, sl)
        for name in ("surface_sigma_field", "surface_pressure_field"):
            got = getattr(loc, name)
            assert got is not None and got.shape == loc.viscosity.shape and got.dtype == np.float32
            assert np.array_equal(got, getattr(sc, name)[sl.g0:sl.g0 + sl.nz_local])
    sc.surface_sigma_field = None                                              # each field is cut on its own
    loc = partition.local_scene(sc, partition.make_slab(sc.nz, 2, 0, p.tileSize))
    assert loc.surface_sigma_field is None and loc.surface_pressure_field is not None
    sc.surface_pressure_field = None
    loc = partition.local_scene(sc, partition.make_slab(sc.nz, 2, 0, p.tileSize))
    assert loc.surface_sigma_field is None and loc.surface_pressure_field is None


def test_brick_cuts_of_both_fields():
    sc, p = _field_scene((32, 32, 32), tile=8)
    for r in range(8):
        b = partition.make_brick((sc.nx, sc.ny, sc.nz), (2, 2, 2), r, p.tileSize)
        loc = partition.local_scene_brick(sc, b)
        ox, oy, oz = b.origin
        nx, ny, nz = b.n_local
        for name in ("surface_sigma_field", "surface_pressure_field"):
            got = getattr(loc, name)
            assert got.shape == (nz, ny, nx)
            assert np.array_equal(got, getattr(sc, name)[oz:oz + nz, oy:oy + ny, ox:ox + nx])
    sc.surface_pressure_field = None
    loc = partition.local_scene_brick(sc, partition.make_brick((sc.nx, sc.ny, sc.nz), (2, 2, 2), 0, p.tileSize))
    assert loc.surface_sigma_field is not None and loc.surface_pressure_field is None


def test_shim_has_the_two_field_rows_empty_by_default():
    src = open(os.path.join(ROOT, "shim", "HDK_PolyStokes_shim.C")).read()
    hdr = open(os.path.join(ROOT, "shim", "HDK_PolyStokes_shim.h")).read()
    for token in ("surfaceSigmaField", "surfacePressureField"):
        m = re.search(r"\{'S',\s*\"%s\",\s*\"[^\"]*\",\s*\"([^\"]*)\",\s*([-0-9.e]+)\}" % token, src)
        assert m and m.group(1) == "" and float(m.group(2)) == 0, token
        assert '"%s"' % token in hdr
    assert "ps_upload_surface_fields(myCtx" in src
    # the GAS helper takes the row and looks the field's name up from it, as for every other field of the node
    assert 'getScalarField(obj, "surfaceSigmaField")' in src and 'getScalarField(obj, "surfacePressureField")' in src
    assert "if (!variableDensity && !surfaceFields) result = polystokes_step(" in src      # neither set: the one call, as before

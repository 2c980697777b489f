"""Free-slip solids (ps_set_solid_boundary) without a GPU: the declaration and export in both libraries, the documented array names,
the Houdini shim's row, and the two floor scenes."""
import ctypes
import os
import re

import numpy as np

from polystokes_amd import _abi as abi
from polystokes_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_point_the_enum_and_the_arrays():
    hdr = open(os.path.join(ROOT, "include", "polystokes.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int32_t\s+ps_set_solid_boundary\s*\(\s*ps_context\s*\*\s*ctx\s*,\s*int32_t\s+mode\s*\)\s*;", code)
    m = re.search(r"enum\s+ps_solid_boundary\s*\{\s*PS_SOLID_NO_SLIP\s*=\s*0\s*,\s*PS_SOLID_FREE_SLIP\s*=\s*1\s*\}\s*;", code)
    assert m
    assert (abi.SOLID_NO_SLIP, abi.SOLID_FREE_SLIP) == (0, 1)
    for name in ('"solidBoundary"', '"solidSlipEdges"'):
        assert name in hdr, name


def test_both_libraries_export_it():
    import polystokes_amd
    assert "ps_set_solid_boundary" in polystokes_amd.EXPORTED_SYMBOLS
    L = polystokes_amd.lib()
    assert hasattr(L, "ps_set_solid_boundary") and L.ps_abi_version() == 1
    assert L.ps_set_solid_boundary(None, abi.SOLID_FREE_SLIP) == abi.FAILED          # no context
    assert L.ps_set_solid_boundary(None, 7) == abi.FAILED
    rel = ctypes.CDLL(os.path.join(ROOT, "polystokes_amd", "libpolystokes_hip_release.so"))
    assert hasattr(rel, "ps_set_solid_boundary")
    rel.ps_set_solid_boundary.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    rel.ps_set_solid_boundary.restype = ctypes.c_int32
    assert rel.ps_set_solid_boundary(None, abi.SOLID_NO_SLIP) == abi.FAILED
    assert polystokes_amd._kind("solidBoundary") == "i" and polystokes_amd._kind("solidSlipEdges") == "i"   # int32 arrays


def test_shim_row_is_off_by_default():
    src = open(os.path.join(ROOT, "shim", "HDK_PolyStokes_shim.C")).read()
    m = re.search(r"\{'T',\s*\"solidFreeSlip\",\s*\"[^\"]*\",\s*nullptr,\s*([-0-9.e]+)\}", src)
    assert m and float(m.group(1)) == 0
    assert "ps_set_solid_boundary(myCtx" in src
    hdr = open(os.path.join(ROOT, "shim", "HDK_PolyStokes_shim.h")).read()
    assert '"solidFreeSlip"' in hdr


def _same(a, b):
    assert a.name == b.name and (a.nx, a.ny, a.nz, a.dx, a.dt, a.density) == (b.nx, b.ny, b.nz, b.dx, b.dt, b.density)
    for f in ("surface", "collision", "viscosity"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    for q in range(3):
        assert np.array_equal(a.vel[q], b.vel[q]) and np.array_equal(a.collisionvel[q], b.collisionvel[q])


def _floor_on_a_face_plane(sc, floor):
    """the collision SDF changes sign exactly on the y-face plane j = floor: solid below, open above, zero on the plane"""
    n = sc.ny
    y = (np.arange(n) + 0.5) * sc.dx
    col = sc.collision[0, :, 0]
    assert np.all(col[y < floor * sc.dx] < 0) and np.all(col[y > floor * sc.dx] > 0)
    assert np.allclose(col, y - floor * sc.dx, atol=1e-6)
    # the plane is a face plane: the cell centres below and above it are half a cell away
    assert np.isclose(-col[floor - 1], 0.5 * sc.dx, rtol=1e-5) and np.isclose(col[floor], 0.5 * sc.dx, rtol=1e-5)
    assert np.all(sc.collision == sc.collision[:1, :, :1])          # the floor spans the grid


def test_sliding_block_scene():
    sc, p = scenes.sliding_block(32, U=2.0)
    _same(sc, scenes.sliding_block(32, U=2.0)[0])
    assert (p.tileSize, p.tilePadding) == (8, 2)
    _floor_on_a_face_plane(sc, 2)
    assert np.all(sc.vel[0] == 2.0) and np.all(sc.vel[1] == 0) and np.all(sc.vel[2] == 0)
    for q in range(3):
        assert np.all(sc.collisionvel[q] == 0)
    inside = sc.surface < 0
    # the liquid box sits on the floor: cells 3 .. 28 in x and z, up to y = 26 cells
    assert inside[16, :26, 16].all() and not inside[16, 26:, 16].any()
    assert inside[3:29, 10, 3:29].all() and not inside[:3, 10, :].any() and not inside[29:, 10, :].any()


def test_moving_floor_scene():
    sc, p = scenes.moving_floor(32, V=0.5)
    _same(sc, scenes.moving_floor(32, V=0.5)[0])
    assert (p.tileSize, p.tilePadding) == (8, 2)
    _floor_on_a_face_plane(sc, 2)
    for q in range(3):
        assert np.all(sc.vel[q] == 0)
    assert np.all(sc.collisionvel[0] == 0.5) and np.all(sc.collisionvel[1] == 0) and np.all(sc.collisionvel[2] == 0)
    assert np.array_equal(sc.surface, scenes.sliding_block(32)[0].surface)

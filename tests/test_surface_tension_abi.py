"""Surface tension (ps_set_surface_tension) without a GPU: the declaration and export in both libraries, the documented array
names, the Houdini shim's two rows, the Python plumbing and the ellipsoid scene."""
import ctypes
import os
import re

import numpy as np

from polystokes_amd import _abi as abi
from polystokes_amd import partition, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_point_and_documents_the_arrays():
    hdr = open(os.path.join(ROOT, "include", "polystokes.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int32_t\s+ps_set_surface_tension\s*\(\s*ps_context\s*\*\s*ctx\s*,\s*double\s+sigma\s*\)\s*;", code)
    for name in ('"surfaceTension"', '"surfaceCurvature"', '"surfaceTensionReducedFaces"'):
        assert name in hdr, name


def test_both_libraries_export_it():
    import polystokes_amd
    assert "ps_set_surface_tension" in polystokes_amd.EXPORTED_SYMBOLS
    L = polystokes_amd.lib()
    assert hasattr(L, "ps_set_surface_tension") and L.ps_abi_version() == 1
    assert L.ps_set_surface_tension(None, 1.0) == abi.FAILED                  # no context
    rel = ctypes.CDLL(os.path.join(ROOT, "polystokes_amd", "libpolystokes_hip_release.so"))
    assert hasattr(rel, "ps_set_surface_tension")


def test_shim_has_the_two_rows_off_by_default():
    src = open(os.path.join(ROOT, "shim", "HDK_PolyStokes_shim.C")).read()
    m = re.search(r"\{'T',\s*\"enableSurfaceTension\",\s*\"[^\"]*\",\s*nullptr,\s*([-0-9.e]+)\}", src)
    assert m and float(m.group(1)) == 0
    m = re.search(r"\{'F',\s*\"surfaceTension\",\s*\"[^\"]*\",\s*nullptr,\s*([-0-9.e]+)\}", src)
    assert m and float(m.group(1)) == 0
    assert "ps_set_surface_tension(myCtx" in src
    hdr = open(os.path.join(ROOT, "shim", "HDK_PolyStokes_shim.h")).read()
    assert '"enableSurfaceTension"' in hdr and '"surfaceTension"' in hdr


def test_scene_carries_sigma_through_the_cuts():
    sc, p = scenes.droplet(32, tile=8)
    assert sc.surface_tension is None
    sc.surface_tension = 0.25
    for r in range(2):
        assert partition.local_scene(sc, partition.make_slab(sc.nz, 2, r, p.tileSize)).surface_tension == 0.25
    b = partition.make_brick((sc.nx, sc.ny, sc.nz), (2, 2, 2), 0, p.tileSize)
    assert partition.local_scene_brick(sc, b).surface_tension == 0.25


def test_ellipsoid_scene():
    n = 32
    sc, p = scenes.ellipsoid_droplet(n, axes=(0.36, 0.26, 0.26), sigma=0.5)
    assert sc.surface_tension == 0.5 and sc.surface.shape == (n, n, n) and sc.surface.dtype == np.float32
    inside = sc.surface < 0
    x = (np.arange(n) + 0.5) / n
    # the liquid is the ellipsoid with semi-axes 0.36 (x), 0.26 (y), 0.26 (z) around the centre
    Z, Y, X = np.meshgrid(x - 0.5, x - 0.5, x - 0.5, indexing="ij")
    assert np.array_equal(inside, (X / 0.36) ** 2 + (Y / 0.26) ** 2 + (Z / 0.26) ** 2 < 1)
    # a distance estimate: unit gradient at the surface
    g = np.gradient(sc.surface.astype(np.float64), 1.0 / n)
    gn = np.sqrt(g[0] ** 2 + g[1] ** 2 + g[2] ** 2)[np.abs(sc.surface) < 0.5 / n]
    assert np.abs(gn - 1).max() < 0.1

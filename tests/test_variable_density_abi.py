"""Variable density (ps_upload_density_field) without a GPU: the declaration and export, the decompositions' cut of a density field,
the Houdini shim's toggle, and the scene helper."""
import os
import re

import numpy as np
import pytest

from polystokes_amd import partition, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_point_and_it_is_exported():
    import polystokes_amd
    hdr = open(os.path.join(ROOT, "include", "polystokes.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int32_t\s+ps_upload_density_field\s*\(\s*ps_context\s*\*\s*ctx\s*,\s*const\s+float\s*\*\s*density\s*\)\s*;", code)
    assert "ps_upload_density_field" in polystokes_amd.EXPORTED_SYMBOLS
    L = polystokes_amd.lib()
    assert hasattr(L, "ps_upload_density_field")
    assert L.ps_abi_version() == 1


def test_refuses_without_a_context():
    import polystokes_amd
    assert polystokes_amd.lib().ps_upload_density_field(None, None) == -1      # PS_FAILED: no context


def _field_scene(n=(24, 20, 64), tile=8):
    sc, p = scenes.blob(*n, seed=3, tile=tile)
    scenes.with_density_field(sc, "smooth", rho0=900.0)
    # mark every cell with its linear index so that any mis-cut shows
    sc.viscosity[:] = np.arange(sc.viscosity.size, dtype=np.float32).reshape(sc.viscosity.shape)
    sc.density_field += sc.viscosity
    return sc, p


@pytest.mark.parametrize("world", [2, 3])
def test_slab_cut_of_a_density_field(world):
    sc, p = _field_scene()
    for r in range(world):
        sl = partition.make_slab(sc.nz, world, r, p.tileSize)
        loc = partition.local_scene(sc, sl)
        assert loc.density_field is not None and loc.density_field.shape == loc.viscosity.shape
        assert np.array_equal(loc.density_field - loc.viscosity, sc.density_field[sl.g0:sl.g0 + sl.nz_local] - sc.viscosity[sl.g0:sl.g0 + sl.nz_local])
        assert np.array_equal(loc.density_field, sc.density_field[sl.g0:sl.g0 + sl.nz_local])
    sc.density_field = None
    assert partition.local_scene(sc, partition.make_slab(sc.nz, 2, 0, p.tileSize)).density_field is None


def test_brick_cut_of_a_density_field():
    sc, p = _field_scene((32, 32, 32), tile=8)
    dims = (2, 2, 2)
    for r in range(8):
        b = partition.make_brick((sc.nx, sc.ny, sc.nz), dims, r, p.tileSize)
        loc = partition.local_scene_brick(sc, b)
        ox, oy, oz = b.origin
        nx, ny, nz = b.n_local
        assert loc.density_field.shape == loc.viscosity.shape == (nz, ny, nx)
        assert np.array_equal(loc.density_field, sc.density_field[oz:oz + nz, oy:oy + ny, ox:ox + nx])
        assert np.array_equal(loc.viscosity, sc.viscosity[oz:oz + nz, oy:oy + ny, ox:ox + nx])
        # the halo block is there: a face on a cut sees both of its cells
        assert all(b.n_local[a] > b.hi[a] - b.lo[a] for a in range(3))


def test_shim_has_the_toggle_and_keeps_the_refusal():
    src = open(os.path.join(ROOT, "shim", "HDK_PolyStokes_shim.C")).read()
    m = re.search(r"\{'T',\s*\"variableDensity\",\s*\"[^\"]*\",\s*nullptr,\s*([-0-9.e]+)\}", src)
    assert m and float(m.group(1)) == 0
    assert '"Variable density is not currently supported"' in src
    assert "ps_upload_density_field(" in src and "toDense(*densityField->getField(), dens)" in src
    assert "VariableDensity" in open(os.path.join(ROOT, "shim", "HDK_PolyStokes_shim.h")).read()


def test_scene_helper_kinds():
    sc, p = scenes.cavity(32)
    scenes.with_density_field(sc, "layers", rho0=2.0, contrast=10.0)
    f = sc.density_field
    assert f.dtype == np.float32 and f.shape == (32, 32, 32)
    k = 32 // 2 + 3
    assert k % p.tileSize != 0                                 # the interface cuts through a tile
    assert np.all(f[:k] == 20.0) and np.all(f[k:] == 2.0)
    scenes.with_density_field(sc, "smooth", rho0=4.0)
    assert len(np.unique(sc.density_field)) > 256 and np.isfinite(sc.density_field).all()
    assert sc.density_field.min() >= 1.0                       # inside the default clamp [1, 1e5]
    with pytest.raises(ValueError):
        scenes.with_density_field(sc, "bubbles")

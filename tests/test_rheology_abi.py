"""Non-Newtonian viscosity (ps_set_rheology) without a GPU: the declaration and export in every library, the documented array names, the
shim rows, and the numpy restatement the GPU tests compare against."""
import ctypes
import os
import re

import numpy as np

import polystokes_amd
from polystokes_amd import _abi as abi

import rheology_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*p):
    with open(os.path.join(ROOT, *p)) as f:
        return f.read()


def test_header_declares_the_setting():
    code = _read("include", "polystokes.h")
    assert re.search(r"int32_t\s+ps_set_rheology\s*\(\s*ps_context\s*\*\s*ctx\s*,\s*const\s+ps_rheology\s*\*\s*r\s*\)\s*;", code)
    assert re.search(r"enum\s+ps_rheology_model\s*\{\s*PS_RHEOLOGY_NEWTONIAN\s*=\s*0\s*,\s*PS_RHEOLOGY_HERSCHEL_BULKLEY\s*=\s*1\s*\}", code)
    m = re.search(r"typedef struct ps_rheology \{(.*?)\} ps_rheology;", code, re.S)
    assert m
    members = re.findall(r"(int32_t|double)\s+(\w+);", m.group(1))
    assert members == [("int32_t", "model"), ("int32_t", "passes"), ("double", "flowIndex"), ("double", "yieldStress"),
                       ("double", "minShearRate"), ("double", "minViscosity"), ("double", "maxViscosity")]
    assert [f[0] for f in abi.Rheology._fields_] == [n for _, n in members]
    for name in ("rheologyModel", "rheologyStrainRate", "rheologyViscosity", "rheologyIterations"):
        assert f'"{name}"' in code, name
    assert "rheology passes need a single domain" in code


def test_every_library_exports_it():
    assert "ps_set_rheology" in polystokes_amd.EXPORTED_SYMBOLS
    L = polystokes_amd.lib()
    assert L.ps_abi_version() == 1
    r = abi.Rheology(abi.RHEOLOGY_HERSCHEL_BULKLEY, 0, 0.5, 1.0, 1e-3, 1e-3, 1e6)
    assert L.ps_set_rheology(None, ctypes.byref(r)) == abi.FAILED          # no context
    assert L.ps_set_rheology(None, None) == abi.FAILED
    for name in ("libpolystokes_hip_release.so", "libpolystokes_hip_affine.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "polystokes_amd", name))
        assert hasattr(lib, "ps_set_rheology"), name
        lib.ps_set_rheology.argtypes = [ctypes.c_void_p, ctypes.POINTER(abi.Rheology)]
        lib.ps_set_rheology.restype = ctypes.c_int32
        assert lib.ps_set_rheology(None, ctypes.byref(r)) == abi.FAILED, name
    assert "ps_rheology.hip" in _read("polystokes_amd", "csrc", "Makefile")


def test_shim_rows_and_call():
    src = _read("shim", "HDK_PolyStokes_shim.C")
    hdr = _read("shim", "HDK_PolyStokes_shim.h")
    rows = {"nonNewtonian": ("T", 0.0), "flowIndex": ("F", 1.0), "yieldStress": ("F", 0.0), "minShearRate": ("F", 1e-3),
            "minViscosity": ("F", 1e-3), "maxViscosity": ("F", 1e6), "rheologyPasses": ("I", 0.0)}
    for name, (kind, default) in rows.items():
        m = re.search(r"\{'(\w)',\s*\"" + name + r"\",\s*\"[^\"]*\",\s*nullptr,\s*([-0-9.e]+)\}", src)
        assert m, name
        assert m.group(1) == kind and float(m.group(2)) == default, (name, m.groups())
        assert f'"{name}"' in hdr, name
    assert "ps_set_rheology(myCtx" in src


def _shear_scene(n=10, gamma=3.0):
    dx = 1.0 / n
    sh = abi.grid_shapes(n, n, n)
    vel = [np.zeros(sh["face" + a], np.float32) for a in "XYZ"]
    y = (np.arange(n) + 0.5) * dx                   # x faces sit at cell-centre heights in y
    vel[0][:] = (gamma * y)[None, :, None]
    used = [np.ones(sh["face" + a], bool) for a in "XYZ"]
    return vel, used, dx


def test_linear_shear_and_rigid_translation():
    gamma = 3.0
    vel, used, dx = _shear_scene(gamma=gamma)
    rate = ref.strain_rate(vel, used, dx)
    inner = rate[:, 1:-1, :]                        # the rows y = 0 and y = n - 1 lack a neighbour in y: G_xy does not exist there
    assert np.allclose(inner, gamma, rtol=1e-6, atol=0), (inner.min(), inner.max())    # D_xy = gamma / 2: sqrt(4 (gamma/2)^2)
    assert np.all(rate[:, 0, :] == 0.0) and np.all(rate[:, -1, :] == 0.0)
    trans = [np.full(v.shape, c, np.float32) for v, c in zip(vel, (1.5, -2.0, 0.25))]
    assert np.array_equal(ref.strain_rate(trans, used, dx), np.zeros_like(rate))
    # the law: Newtonian limit exact, power law, Bingham
    K = np.full(inner.shape, 7.0, np.float32)
    assert np.array_equal(ref.viscosity(inner, K, 1.0, 0.0, 1e-3, 1e-3, 1e6), K.astype(np.float64))
    assert np.allclose(ref.viscosity(inner, K, 0.5, 0.0, 1e-3, 1e-3, 1e6), 7.0 / np.sqrt(gamma))
    assert np.allclose(ref.viscosity(inner, K, 1.0, 2.0, 1e-3, 1e-3, 1e6), 7.0 + 2.0 / gamma)
    assert np.all(ref.viscosity(np.zeros_like(inner), K, 1.0, 2.0, 1e-3, 1e-3, 1e3) == 1e3)          # clamped at rest


def _brute(vel, used, dx):
    """the definition, one cell at a time"""
    nz, ny, nx = vel[0].shape[0], vel[0].shape[1], vel[0].shape[2] - 1
    n = (nx, ny, nz)
    out = np.zeros((nz, ny, nx))
    pairs = np.zeros((3, nz, ny, nx), bool)

    def at(a, f):
        return f[2], f[1], f[0]

    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                c = (i, j, k)
                D = [0.0] * 3
                G = {}
                for a in range(3):
                    f0 = list(c)
                    f1 = list(c)
                    f1[a] += 1
                    if used[a][at(a, f0)] and used[a][at(a, f1)]:
                        pairs[a, k, j, i] = True
                        D[a] = (float(vel[a][at(a, f1)]) - float(vel[a][at(a, f0)])) / dx
                    for b in range(3):
                        if b == a:
                            continue
                        vals = []
                        for f in (f0, f1):
                            lo, hi = list(f), list(f)
                            lo[b] -= 1
                            hi[b] += 1
                            if lo[b] < 0 or hi[b] >= n[b]:
                                continue
                            if used[a][at(a, lo)] and used[a][at(a, hi)]:
                                vals.append((float(vel[a][at(a, hi)]) - float(vel[a][at(a, lo)])) / (2.0 * dx))
                        G[(a, b)] = 0.5 * (vals[0] + vals[1]) if len(vals) == 2 else (vals[0] if vals else 0.0)
                Dxy, Dxz, Dyz = 0.5 * (G[(0, 1)] + G[(1, 0)]), 0.5 * (G[(0, 2)] + G[(2, 0)]), 0.5 * (G[(1, 2)] + G[(2, 1)])
                out[k, j, i] = np.sqrt(2.0 * (D[0] * D[0] + D[1] * D[1] + D[2] * D[2]) + 4.0 * (Dxy * Dxy + Dxz * Dxz + Dyz * Dyz))
    return out, pairs


def test_masks_cover_every_used_pair():
    rng = np.random.RandomState(3)
    nx, ny, nz = 7, 5, 6
    sh = abi.grid_shapes(nx, ny, nz)
    vel = [rng.standard_normal(sh["face" + a]).astype(np.float32) for a in "XYZ"]
    used = [rng.uniform(size=sh["face" + a]) < 0.7 for a in "XYZ"]
    dx = 0.125
    want, pairs = _brute(vel, used, dx)
    D, G, pair, has = ref.masks_and_gradients(vel, used, dx)
    for a in range(3):
        assert np.array_equal(pair[a], pairs[a]), a              # every cell with a used face pair, and no other
        assert np.all(D[a][~pair[a]] == 0.0)
        for b in range(3):
            if b != a:
                assert np.all(G[(a, b)][~has[(a, b)]] == 0.0)
    got = ref.strain_rate(vel, used, dx)
    assert np.allclose(got, want, rtol=1e-13, atol=0)
    assert np.all(ref.ulps(got.astype(np.float32), want.astype(np.float32)) <= 1)

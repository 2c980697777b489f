"""ps_set_velocity_extrapolation at the product boundary, without a GPU: the header declares the entry point and its limit, every library
exports the symbol and refuses a null context, the Python layer carries it, the Houdini shim has its row, off by default."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*p):
    with open(os.path.join(ROOT, *p)) as f:
        return f.read()


def test_header_declares_the_entry_point_and_the_limit():
    hdr = _read("include", "polystokes.h")
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int32_t\s+ps_set_velocity_extrapolation\s*\(\s*ps_context\s*\*\s*ctx\s*,\s*int32_t\s+layers\s*\)\s*;", code)
    assert re.search(r"#define\s+PS_EXTRAPOLATION_MAX_LAYERS\s+64\b", code)
    for name in ("velocityExtrapolation", "extrapolationLayerX", "extrapolationLayerY", "extrapolationLayerZ", "extrapolationCounts"):
        assert '"%s"' % name in hdr, name
    assert "layers outside 0..64" in hdr
    assert "(nx+1) ny nz + nx (ny+1) nz + nx ny (nz+1) bytes" in hdr                 # the memory the GPU test asserts is stated
    body = code[code.index("typedef struct ps_params {"):code.index("} ps_params;")]
    assert "xtrapol" not in body                                                     # a context setting, not a ps_params member
    assert re.search(r"PS_STAGE_COUNT\s*=\s*11\b", code)


def test_every_library_exports_it_and_refuses_a_null_context():
    import polystokes_amd
    from polystokes_amd import _abi as abi
    assert "ps_set_velocity_extrapolation" in polystokes_amd.EXPORTED_SYMBOLS
    L = polystokes_amd.lib()
    assert L.ps_abi_version() == 1
    assert L.ps_set_velocity_extrapolation(None, 3) == abi.FAILED
    assert L.ps_set_velocity_extrapolation(None, 1000) == abi.FAILED
    for name in ("libpolystokes_hip_release.so", "libpolystokes_hip_affine.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "polystokes_amd", name))
        assert hasattr(lib, "ps_set_velocity_extrapolation"), name
        lib.ps_set_velocity_extrapolation.argtypes = [ctypes.c_void_p, ctypes.c_int32]
        lib.ps_set_velocity_extrapolation.restype = ctypes.c_int32
        assert lib.ps_set_velocity_extrapolation(None, 3) == abi.FAILED, name
        lib.ps_abi_version.restype = ctypes.c_int32
        assert lib.ps_abi_version() == 1, name
    assert "ps_extrapolate.hip" in _read("polystokes_amd", "csrc", "Makefile")


def test_python_layer_carries_it():
    import numpy as np
    import polystokes_amd
    from polystokes_amd import _abi as abi
    assert abi.EXTRAPOLATION_MAX_LAYERS == 64
    assert callable(polystokes_amd.Solver.set_velocity_extrapolation) and callable(polystokes_amd.Group.set_velocity_extrapolation)
    L = polystokes_amd.lib()
    assert L.ps_set_velocity_extrapolation.restype is ctypes.c_int32 and len(L.ps_set_velocity_extrapolation.argtypes) == 2
    for name in ("velocityExtrapolation", "extrapolationLayerX", "extrapolationLayerY", "extrapolationLayerZ", "extrapolationCounts"):
        assert polystokes_amd._kind(name) == "i", name
    assert polystokes_amd._DT[(1, "i")] is np.int8 and polystokes_amd._DT[(4, "i")] is np.int32


def test_shim_row_is_off_by_default():
    src = _read("shim", "HDK_PolyStokes_shim.C")
    m = re.search(r"\{'(\w)',\s*\"extrapolateLayers\",\s*\"[^\"]*\",\s*nullptr,\s*([-0-9.e]+)\}", src)
    assert m and m.group(1) == "I" and float(m.group(2)) == 0.0
    assert "ps_set_velocity_extrapolation(myCtx" in src
    assert '"extrapolateLayers"' in _read("shim", "HDK_PolyStokes_shim.h")

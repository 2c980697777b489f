"""Collider loads at the product boundary, without a GPU: the header declares the calls, the arrays and the limit, every library exports
the symbols and refuses a null context, the Python layer carries them, the Makefile lists the file, the Houdini shim has its row."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ps_set_collider_loads", "ps_upload_collider_ids", "ps_upload_collider_ids_device", "ps_get_collider_loads",
           "ps_get_collider_loads_device")
ARRAYS = ("colliderLoads", "colliderForce", "colliderTorque", "colliderLoadTerms", "colliderLoadScale")


def _read(*p):
    with open(os.path.join(ROOT, *p)) as f:
        return f.read()


def test_header_declares_the_calls_the_arrays_and_the_limit():
    hdr = _read("include", "polystokes.h")
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"#define\s+PS_COLLIDER_MAX\s+64\b", code)
    assert re.search(r"typedef\s+struct\s+ps_collider_loads\s*\{\s*int32_t\s+count\s*;\s*const\s+double\s*\*\s*pivots\s*;\s*\}\s*ps_collider_loads\s*;", code)
    assert re.search(r"int32_t\s+ps_set_collider_loads\s*\(\s*ps_context\s*\*\s*\w+\s*,\s*const\s+ps_collider_loads\s*\*\s*\w+\s*\)\s*;", code)
    assert re.search(r"int32_t\s+ps_upload_collider_ids\s*\(\s*ps_context\s*\*\s*\w+\s*,\s*const\s+int32_t\s*\*\s*\w+\s*\)\s*;", code)
    assert re.search(r"int32_t\s+ps_upload_collider_ids_device\s*\(\s*ps_context\s*\*\s*\w+\s*,\s*const\s+int32_t\s*\*\s*\w+\s*,\s*int32_t\s+layout\s*,\s*void\s*\*\s*stream\s*\)\s*;", code)
    assert re.search(r"int32_t\s+ps_get_collider_loads\s*\(\s*ps_context\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*,\s*int64_t\s+\w+\s*\)\s*;", code)
    assert re.search(r"int32_t\s+ps_get_collider_loads_device\s*\(\s*ps_context\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*,\s*int64_t\s+\w+\s*,\s*void\s*\*\s*stream\s*\)\s*;", code)
    for name in ARRAYS:
        assert '"%s"' % name in hdr, name
    assert "count outside 0..64" in hdr
    assert "W * (100 * count + 12) bytes" in hdr and "172 * count + 4 bytes" in hdr      # the memory the GPU test asserts is stated
    body = code[code.index("typedef struct ps_params {"):code.index("} ps_params;")]
    assert "ollider" not in body                                                        # a context setting, not a ps_params member
    assert re.search(r"PS_STAGE_COUNT\s*=\s*11\b", code)


def test_every_library_exports_them_and_refuses_a_null_context():
    import polystokes_amd
    from polystokes_amd import _abi as abi
    for sym in SYMBOLS:
        assert sym in polystokes_amd.EXPORTED_SYMBOLS, sym
    L = polystokes_amd.lib()
    assert L.ps_abi_version() == 1
    libs = [L] + [ctypes.CDLL(os.path.join(ROOT, "polystokes_amd", n)) for n in ("libpolystokes_hip_release.so", "libpolystokes_hip_affine.so")]
    setting = abi.ColliderLoads(3, None)
    out = (ctypes.c_double * 18)()
    for lib in libs:
        for sym in SYMBOLS:
            assert hasattr(lib, sym), sym
            getattr(lib, sym).restype = ctypes.c_int32
        lib.ps_set_collider_loads.argtypes = [ctypes.c_void_p, ctypes.POINTER(abi.ColliderLoads)]
        lib.ps_upload_collider_ids.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        lib.ps_upload_collider_ids_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
        lib.ps_get_collider_loads.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
        lib.ps_get_collider_loads_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
        assert lib.ps_set_collider_loads(None, ctypes.byref(setting)) == abi.FAILED
        assert lib.ps_upload_collider_ids(None, None) == abi.FAILED
        assert lib.ps_upload_collider_ids_device(None, None, 0, None) == abi.FAILED
        assert lib.ps_get_collider_loads(None, out, 18) == abi.FAILED
        assert lib.ps_get_collider_loads_device(None, None, 18, None) == abi.FAILED
        lib.ps_abi_version.restype = ctypes.c_int32
        assert lib.ps_abi_version() == 1
    assert "ps_loads.hip" in _read("polystokes_amd", "csrc", "Makefile")


def test_python_layer_carries_them():
    import numpy as np
    import polystokes_amd
    from polystokes_amd import _abi as abi
    assert abi.COLLIDER_MAX == 64
    assert ctypes.sizeof(abi.ColliderLoads) == 16 and abi.ColliderLoads.pivots.offset == 8
    for name in ("set_collider_loads", "upload_collider_ids", "upload_collider_ids_device", "collider_loads", "collider_loads_device"):
        assert callable(getattr(polystokes_amd.Solver, name)), name
    assert callable(polystokes_amd.Group.set_collider_loads)
    for name in ("colliderLoads", "colliderLoadTerms"):
        assert polystokes_amd._kind(name) == "i", name
    for name in ("colliderForce", "colliderTorque", "colliderLoadScale"):
        assert polystokes_amd._kind(name) == "f", name
    assert polystokes_amd._DT[(8, "f")] is np.float64


def test_shim_row_is_off_by_default():
    src = _read("shim", "HDK_PolyStokes_shim.C")
    m = re.search(r"\{'(\w)',\s*\"colliderLoads\",\s*\"[^\"]*\",\s*nullptr,\s*([-0-9.e]+)\}", src)
    assert m and m.group(1) == "I" and float(m.group(2)) == 0.0
    assert "ps_set_collider_loads(myCtx" in src
    assert '"colliderLoads"' in _read("shim", "HDK_PolyStokes_shim.h")

"""Air pockets at the product boundary, without a GPU: the header declares the five calls and states the definition, the arrays and the
memory; every library exports the symbols and refuses what needs no device work; the Python layer carries them; the Makefile lists the file."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ps_label_air_pockets", "ps_get_air_pockets", "ps_download_air_pocket_ids", "ps_download_air_pocket_ids_device",
           "ps_set_air_pocket_pressures")
ARRAYS = ("airPockets", "airPocketIds", "airPocketUnits", "airPocketCells", "airPocketOpen", "airPocketVolume", "airPocketPasses")


def _read(*p):
    with open(os.path.join(ROOT, *p)) as f:
        return f.read()


def test_header_declares_the_calls_and_states_the_definition():
    hdr = _read("include", "polystokes.h")
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    ctx = r"ps_context\s*\*\s*\w+"
    assert re.search(r"int32_t\s+ps_label_air_pockets\s*\(\s*" + ctx + r"\s*,\s*int32_t\s*\*\s*\w+\s*\)\s*;", code)
    assert re.search(r"int32_t\s+ps_get_air_pockets\s*\(\s*" + ctx + r"\s*,\s*double\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*,\s*int64_t\s+\w+\s*\)\s*;", code)
    assert re.search(r"int32_t\s+ps_download_air_pocket_ids\s*\(\s*" + ctx + r"\s*,\s*int32_t\s*\*\s*\w+\s*\)\s*;", code)
    assert re.search(r"int32_t\s+ps_download_air_pocket_ids_device\s*\(\s*" + ctx + r"\s*,\s*int32_t\s*\*\s*\w+\s*,\s*int32_t\s+layout\s*,\s*void\s*\*\s*stream\s*\)\s*;", code)
    assert re.search(r"int32_t\s+ps_set_air_pocket_pressures\s*\(\s*" + ctx + r"\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*int64_t\s+\w+\s*\)\s*;", code)
    assert code.index("ps_get_collider_loads(") < code.index("ps_label_air_pockets(") < code.index("polystokes_step(")   # after the collider loads
    for name in ARRAYS:
        assert '"%s"' % name in hdr, name
    for needle in ("fw_c > 0 and lw_c <= 0.5", "llrint((double)fw_c * (1.0 - (double)lw_c) * 1048576.0)",
                   "((double)units_k * (1.0 / 1048576.0)) * (dx * dx * dx)", "-x, +x, -y, +y, -z, +z", "air pockets need a single domain",
                   "pressure of pocket N is not finite", "never see pockets", "24 * K bytes", "ps_memory_stats entry 2 is 0"):
        assert needle in hdr, needle
    body = code[code.index("typedef struct ps_params {"):code.index("} ps_params;")]
    assert "ocket" not in body                                                          # calls on a context, not ps_params members


def _typed(lib):
    from polystokes_amd import _abi as abi
    for name, argtypes in abi.AIR_POCKET_CALLS:
        assert hasattr(lib, name), name
        getattr(lib, name).argtypes = list(argtypes)
        getattr(lib, name).restype = ctypes.c_int32
    return lib


def test_every_library_exports_them_and_refuses_a_null_context():
    import polystokes_amd
    from polystokes_amd import _abi as abi
    assert tuple(n for n, _ in abi.AIR_POCKET_CALLS) == SYMBOLS
    for sym in SYMBOLS:
        assert sym in polystokes_amd.EXPORTED_SYMBOLS, sym
    L = polystokes_amd.lib()
    libs = [L] + [ctypes.CDLL(os.path.join(ROOT, "polystokes_amd", n)) for n in ("libpolystokes_hip_release.so", "libpolystokes_hip_affine.so")]
    k = ctypes.c_int32(7)
    vol = (ctypes.c_double * 4)()
    opn = (ctypes.c_int32 * 4)()
    for lib in libs:
        _typed(lib)
        assert lib.ps_label_air_pockets(None, ctypes.byref(k)) == abi.FAILED and k.value == 7
        assert lib.ps_get_air_pockets(None, vol, opn, 4) == abi.FAILED
        assert lib.ps_download_air_pocket_ids(None, opn) == abi.FAILED
        assert lib.ps_download_air_pocket_ids_device(None, None, 0, None) == abi.FAILED
        assert lib.ps_set_air_pocket_pressures(None, vol, 4) == abi.FAILED
        lib.ps_abi_version.restype = ctypes.c_int32
        assert lib.ps_abi_version() == 1
    mk = _read("polystokes_amd", "csrc", "Makefile")
    assert "ps_pockets.hip" in mk and "ps_loads.hip ps_pockets.hip" in mk              # in the one list all three libraries build from
    assert "getenv" not in _read("polystokes_amd", "csrc", "ps_pockets.hip") and "PS_ENV" not in _read("polystokes_amd", "csrc", "ps_pockets.hip")


def test_the_propagation_kernels_have_one_copy():
    """k_cc_step and k_cc_local serve the REDUCED regions and the pockets from one header"""
    shared = _read("polystokes_amd", "csrc", "ps_kernels_cc.hpp")
    for kernel in ("k_cc_step", "k_cc_local"):
        assert len(re.findall(r"__global__[^;{]*\b%s\s*\(" % kernel, shared)) == 1, kernel
        for src in ("ps_grid.hip", "ps_pockets.hip"):
            text = _read("polystokes_amd", "csrc", src)
            assert '#include "ps_kernels_cc.hpp"' in text and kernel in text, (src, kernel)
            assert not re.search(r"__global__[^;{]*\b%s\s*\(" % kernel, text), (src, kernel)


def test_python_layer_carries_them():
    import numpy as np
    import polystokes_amd
    for name in ("label_air_pockets", "air_pockets", "air_pocket_ids", "air_pocket_ids_device", "set_air_pocket_pressures"):
        assert callable(getattr(polystokes_amd.Solver, name)), name
    for name in ARRAYS:
        assert polystokes_amd._kind(name) == ("f" if name == "airPocketVolume" else "i"), name
    assert polystokes_amd._DT[(8, "i")] is np.int64 and polystokes_amd._DT[(8, "f")] is np.float64


def test_documents_describe_it():
    assert "ps_label_air_pockets" in _read("README.md")
    assert re.search(r"^#+ .*Air pockets", _read("DESIGN.md"), flags=re.M)
    assert os.path.exists(os.path.join(ROOT, "profiles", "air_pockets.md"))

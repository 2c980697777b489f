"""Advection at the product boundary, without a GPU: the header declares the macro, the struct and the two calls and states the rule, the
refusals, the arrays and the memory; every library exports the symbols and refuses a null context; the Python layer's struct has the
header's size and offsets; the Makefile lists the file; the documents describe the call."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ps_advect_fields", "ps_advect_fields_device")
ARRAYS = ("advection", "advectionStep", "advectionCounts")


def _read(*p):
    with open(os.path.join(ROOT, *p)) as f:
        return f.read()


def test_header_declares_the_calls_and_states_the_rule():
    hdr = _read("include", "polystokes.h")
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    ctx = r"ps_context\s*\*\s*\w+"
    assert re.search(r"#define\s+PS_ADVECT_MAX_CELL_FIELDS\s+8\b", code)
    assert re.search(r"typedef\s+struct\s+ps_advection\s*\{\s*double\s+dt\s*;\s*int32_t\s+order\s*;\s*int32_t\s+cellFields\s*;\s*const\s+float\s*\*\s*carrier\[3\]\s*;"
                     r"\s*const\s+float\s*\*\s*cellIn\[PS_ADVECT_MAX_CELL_FIELDS\]\s*;\s*float\s*\*\s*cellOut\[PS_ADVECT_MAX_CELL_FIELDS\]\s*;"
                     r"\s*float\s*\*\s*velOut\[3\]\s*;\s*\}\s*ps_advection\s*;", code)
    assert re.search(r"int32_t\s+ps_advect_fields\s*\(\s*" + ctx + r"\s*,\s*const\s+ps_advection\s*\*\s*\w+\s*\)\s*;", code)
    assert re.search(r"int32_t\s+ps_advect_fields_device\s*\(\s*" + ctx + r"\s*,\s*const\s+ps_advection\s*\*\s*\w+\s*,\s*int32_t\s+layout\s*,\s*void\s*\*\s*stream\s*\)\s*;", code)
    assert (code.index("ps_download_fields_device(") < code.index("PS_ADVECT_MAX_CELL_FIELDS") < code.index("typedef struct ps_advection")
            < code.index("ps_advect_fields(") < code.index("ps_advect_fields_device("))      # after the device-resident calls it follows
    for name in ARRAYS:
        assert '"%s"' % name in hdr, name
    flat = re.sub(r"\n \* *", " ", hdr)                                                  # (a comment's line breaks fall where they fall)
    for needle in ("p0_m = (double)i_m + o_m", "s_m = p_m - o_m", "c_m = min(max(s_m, 0.0), (double)(d_m - 1))", "l_m = (int)floor(c_m)",
                   "h_m = min(l_m + 1, d_m - 1)", "f_m = c_m - (double)l_m", "lo + (hi - lo) * f", "U(p) = (Smp(C_0, 1, p), Smp(C_1, 2, p), Smp(C_2, 3, p))",
                   "r = dt / dx", "p1_m = p0_m - r * U_m(p0)", "pm_m = p0_m - (0.5 * r) * U_m(p0)", "p1_m = p0_m - r * U_m(pm)",
                   "counted in slot 4", "(float)Smp(cellIn[q], 0, p1)", "(float)Smp(C_a, 1 + a, p1)", "0x7fc00000", "s_m < 0 or s_m > d_m - 1",
                   "computed once", "order outside 1..2", "cellFields outside 0..8", "dt not finite", "carrier partly null", "velOut partly null",
                   "nothing to do", "output N overlaps input M", "output N overlaps output M", "advection needs a single domain",
                   "no written velocity since the upload", "20 bytes", "ps_memory_stats entry 2 is 0", "does not synchronise the host", "Out of scope",
                   "MacCormack", "in-place operation"):
        assert needle in flat, needle
    body = code[code.index("typedef struct ps_params {"):code.index("} ps_params;")]
    assert "dvect" not in body                                                          # a call on a context, not a ps_params member


def test_every_library_exports_them_and_refuses_a_null_context():
    import polystokes_amd
    from polystokes_amd import _abi as abi
    assert tuple(n for n, _ in abi.ADVECTION_CALLS) == SYMBOLS
    for sym in SYMBOLS:
        assert sym in polystokes_amd.EXPORTED_SYMBOLS, sym
    L = polystokes_amd.lib()
    libs = [L] + [ctypes.CDLL(os.path.join(ROOT, "polystokes_amd", n)) for n in ("libpolystokes_hip_release.so", "libpolystokes_hip_affine.so")]
    A = abi.Advection()
    A.dt, A.order, A.cellFields = 0.1, 1, 0
    for lib in libs:
        for name, argtypes in abi.ADVECTION_CALLS:
            assert hasattr(lib, name), name
            getattr(lib, name).argtypes = list(argtypes)
            getattr(lib, name).restype = ctypes.c_int32
        assert lib.ps_advect_fields(None, ctypes.byref(A)) == abi.FAILED
        assert lib.ps_advect_fields_device(None, ctypes.byref(A), 0, None) == abi.FAILED
    mk = _read("polystokes_amd", "csrc", "Makefile")
    assert re.search(r"^SRC := .*\bps_advect\.hip\b", mk, flags=re.M)                   # in the one list all three libraries build from
    src = _read("polystokes_amd", "csrc", "ps_advect.hip")
    assert "getenv" not in src and "PS_ENV" not in src                                 # no switch
    assert "waveBinAdd(" in src and "atomicAdd(&T.counts" in src and not re.search(r"atomicAdd\([^;]*(float|double)", src)   # integer counters only
    assert src.count("hipLaunchKernelGGL(") == 1                                        # one launch covers the four grids


def test_python_struct_has_the_headers_size_and_offsets(tmp_path):
    """the header's own layout, from the compiler that builds the oracle, against the ctypes mirror"""
    import polystokes_amd
    from polystokes_amd import _abi as abi
    names = [n for n, _ in abi.Advection._fields_]
    assert names == ["dt", "order", "cellFields", "carrier", "cellIn", "cellOut", "velOut"]
    prog = tmp_path / "layout.cpp"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "polystokes.h"\nint main(void) {\n    printf("%zu", sizeof(ps_advection));\n'
                    + "".join('    printf(" %%zu", offsetof(ps_advection, %s));\n' % n for n in names)
                    + '    printf(" %d\\n", PS_ADVECT_MAX_CELL_FIELDS);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [ctypes.sizeof(abi.Advection)] + [getattr(abi.Advection, n).offset for n in names] + [abi.ADVECT_MAX_CELL_FIELDS]
    assert got == want, (got, want)
    assert want == [192, 0, 8, 12, 16, 40, 104, 168, 8]
    for name in ("advect", "advect_device", "advection"):
        assert callable(getattr(polystokes_amd.Solver, name)), name
    for name in ("advection", "advectionCounts"):
        assert polystokes_amd._kind(name) == "i", name
    assert polystokes_amd._kind("advectionStep") == "f"


def test_documents_describe_it():
    assert "ps_advect_fields" in _read("README.md")
    design = _read("DESIGN.md")
    heads = [m.group(1).strip() for m in re.finditer(r"^#+ (.*)$", design, flags=re.M)]
    assert any(h.endswith("Advection") or h.startswith("Advection") for h in heads), heads[-10:]
    integration = _read("INTEGRATION.md")
    assert "ps_advect_fields_device" in integration
    loop = integration[integration.index("ps_advect_fields_device") - 1500:integration.index("ps_advect_fields_device") + 1500]
    for step in ("upload", "place", "paint", "step", "loads", "advect"):
        assert step in loop, step
    assert os.path.exists(os.path.join(ROOT, "profiles", "advection.md"))
    assert os.path.exists(os.path.join(ROOT, "scripts", "advection_ab.py"))

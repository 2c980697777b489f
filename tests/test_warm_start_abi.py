"""CPU-side checks of the warm-start boundary (ps_set_warm_start, ps_download_solution_fields): declared in the public header, exported by
the lab and release libraries, mirrored by the Python harness, reachable from the Houdini shim's template."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ps_set_warm_start", "ps_download_solution_fields")


def _header():
    return open(os.path.join(ROOT, "include", "polystokes.h")).read()


def _header_symbols():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return set(re.findall(r"\b(ps_[a-z_]+|polystokes_step)\s*\(", txt))


def test_header_declares_the_entry_points_and_the_struct():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"int32_t\s+ps_set_warm_start\s*\(\s*ps_context\s*\*\s*ctx\s*,\s*int32_t\s+mode\s*\)\s*;", txt)
    assert re.search(r"int32_t\s+ps_download_solution_fields\s*\(\s*ps_context\s*\*\s*ctx\s*,\s*const\s+ps_solution_out\s*\*\s*out\s*\)\s*;", txt)
    assert re.search(r"PS_WARM_NONE\s*=\s*0\s*,\s*PS_WARM_PREVIOUS_STEP\s*=\s*1", txt)
    body = txt[txt.index("typedef struct ps_solution_out {"):txt.index("} ps_solution_out;")]
    members = re.findall(r"float\s*\*\s*(\w+)(\[3\])?\s*;", body)
    assert [(m, d) for m, d in members] == [("pressure", ""), ("tauDiag", "[3]"), ("tauEdge", "[3]")]


def test_exported_symbols_match_the_header():
    import polystokes_amd
    assert set(NEW_SYMBOLS) <= _header_symbols()
    assert set(polystokes_amd.EXPORTED_SYMBOLS) == _header_symbols()


def test_lab_and_release_libraries_export_them():
    import polystokes_amd
    L = polystokes_amd.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s), s
    rel = os.path.join(ROOT, "polystokes_amd", "libpolystokes_hip_release.so")
    assert os.path.exists(rel), "build it: make -C polystokes_amd/csrc"
    R = ctypes.CDLL(rel)
    for s in NEW_SYMBOLS:
        assert hasattr(R, s), s


def test_null_context_is_refused():
    import polystokes_amd
    L = polystokes_amd.lib()
    assert L.ps_set_warm_start(None, 1) == -1
    assert L.ps_download_solution_fields(None, None) == -1


def test_ctypes_struct_matches_the_header():
    from polystokes_amd import _abi as abi
    names = [f[0] for f in abi.SolutionOut._fields_]
    assert names == ["pressure", "tauDiag", "tauEdge"]
    assert ctypes.sizeof(abi.SolutionOut) == 7 * ctypes.sizeof(ctypes.c_void_p)
    assert abi.SolutionOut.tauDiag.offset == ctypes.sizeof(ctypes.c_void_p)
    assert abi.SolutionOut.tauEdge.offset == 4 * ctypes.sizeof(ctypes.c_void_p)
    assert (abi.WARM_NONE, abi.WARM_PREVIOUS_STEP) == (0, 1)
    assert [g for _, g in abi.SOLUTION_FIELDS] == ["center"] * 4 + ["edgeYZ", "edgeXZ", "edgeXY"]


def test_solver_wrapper_offers_the_feature():
    import polystokes_amd
    assert callable(getattr(polystokes_amd.Solver, "set_warm_start", None))
    assert callable(getattr(polystokes_amd.Solver, "solution_fields", None))


def test_shim_rows_exist_with_default_zero():
    src = open(os.path.join(ROOT, "shim", "HDK_PolyStokes_shim.C")).read()
    rows = {}
    for m in re.finditer(r"\{'([SFITO])',\s*(\"[^\"]+\"|[A-Z_]+),\s*\"[^\"]*\",\s*(nullptr|\"(?:[^\"\\]|\\.)*\"),\s*([-0-9.e]+)\}", src):
        rows[m.group(2).strip('"')] = (m.group(1), float(m.group(4)))
    assert rows.get("warmStartPreviousStep") == ("T", 0.0)
    assert rows.get("writePressureField") == ("T", 0.0)
    assert rows.get("useWarmStart") == ("T", 1.0)          # the reference's toggle keeps its meaning and default
    assert "ps_set_warm_start(" in src and "ps_download_solution_fields(" in src
    hdr = open(os.path.join(ROOT, "shim", "HDK_PolyStokes_shim.h")).read()
    assert '"warmStartPreviousStep"' in hdr and '"writePressureField"' in hdr

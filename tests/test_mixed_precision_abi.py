"""ps_set_solve_precision at the product boundary, without a GPU: the header declares the entry point and its enum, the Python layer
carries them, the library exports the symbol and refuses a null context."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _code():
    hdr = open(os.path.join(ROOT, "include", "polystokes.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), hdr


def test_header_declares_the_entry_point_and_the_enum():
    code, hdr = _code()
    assert re.search(r"int32_t\s+ps_set_solve_precision\s*\(\s*ps_context\s*\*\s*ctx\s*,\s*int32_t\s+mode\s*\)\s*;", code)
    assert re.search(r"enum\s+ps_solve_precision\s*\{\s*PS_PRECISION_FP64\s*=\s*0\s*,\s*PS_PRECISION_MIXED\s*=\s*1\s*\}\s*;", code)
    for name in ("solvePrecisionUsed", "solvePassIterations", "solveTrueResidual"):      # the arrays are documented with the entry point
        assert '"%s"' % name in hdr, name
    # no new ps_params member: the setting is a context setting (the shim's table test covers that struct)
    body = code[code.index("typedef struct ps_params {"):code.index("} ps_params;")]
    assert "recision" not in body


def test_python_layer_carries_them():
    import polystokes_amd
    from polystokes_amd import _abi as abi
    assert "ps_set_solve_precision" in polystokes_amd.EXPORTED_SYMBOLS
    assert (abi.PRECISION_FP64, abi.PRECISION_MIXED) == (0, 1)
    assert callable(polystokes_amd.Solver.set_solve_precision) and callable(polystokes_amd.Group.set_solve_precision)
    L = polystokes_amd.lib()
    assert L.ps_set_solve_precision.restype is not None and len(L.ps_set_solve_precision.argtypes) == 2
    assert polystokes_amd._kind("solvePrecisionUsed") == "i" and polystokes_amd._kind("solvePassIterations") == "i"
    assert polystokes_amd._kind("solveTrueResidual") == "f"
    assert L.ps_abi_version() == 1


def test_null_context_is_refused():
    import polystokes_amd
    from polystokes_amd import _abi as abi
    L = polystokes_amd.lib()
    assert L.ps_set_solve_precision(None, abi.PRECISION_MIXED) == abi.FAILED
    assert L.ps_set_solve_precision(None, 7) == abi.FAILED

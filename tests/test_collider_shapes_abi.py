"""Collider shapes at the product boundary, without a GPU: the header declares the structs and the three calls between the collider motions
and the air pockets and states the rule, the refusals, the arrays and the memory; every library exports the symbols and refuses a null
context; the Python layer carries them; the Makefile lists the file; the documents describe it."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ps_set_collider_shapes", "ps_place_colliders", "ps_place_colliders_device")
ARRAYS = ("colliderShapes", "colliderPlacement", "colliderPoseTable", "colliderPlacedCells", "collisionField", "colliderCellIds")


def _read(*p):
    with open(os.path.join(ROOT, *p)) as f:
        return f.read()


def test_header_declares_the_calls_in_their_place_and_states_the_rule():
    hdr = _read("include", "polystokes.h")
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    ctx = r"ps_context\s*\*\s*\w+"
    assert re.search(r"#define\s+PS_COLLIDER_SHAPE_REACH\s+4\.0\b", code)
    assert re.search(r"typedef\s+struct\s+ps_collider_shape\s*\{\s*int32_t\s+n\[3\]\s*;\s*int32_t\s+reserved\s*;\s*double\s+h\s*;\s*double\s+orig\[3\]\s*;"
                     r"\s*const\s+float\s*\*\s*sdf\s*;\s*\}\s*ps_collider_shape\s*;", code)
    assert re.search(r"typedef\s+struct\s+ps_collider_shapes\s*\{\s*int32_t\s+count\s*;\s*const\s+ps_collider_shape\s*\*\s*shape\s*;\s*\}\s*ps_collider_shapes\s*;", code)
    assert re.search(r"typedef\s+struct\s+ps_collider_poses\s*\{\s*int32_t\s+count\s*;\s*const\s+double\s*\*\s*pose\s*;\s*\}\s*ps_collider_poses\s*;", code)
    assert re.search(r"int32_t\s+ps_set_collider_shapes\s*\(\s*" + ctx + r"\s*,\s*const\s+ps_collider_shapes\s*\*\s*\w+\s*\)\s*;", code)
    assert re.search(r"int32_t\s+ps_place_colliders\s*\(\s*" + ctx + r"\s*,\s*const\s+ps_collider_poses\s*\*\s*\w+\s*\)\s*;", code)
    assert re.search(r"int32_t\s+ps_place_colliders_device\s*\(\s*" + ctx + r"\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*void\s*\*\s*stream\s*\)\s*;", code)
    # directly after the collider motions, before the air pockets
    assert (code.index("ps_paint_collider_velocities_device(") < code.index("PS_COLLIDER_SHAPE_REACH") < code.index("typedef struct ps_collider_shape ")
            < code.index("ps_set_collider_shapes(") < code.index("typedef struct ps_collider_poses") < code.index("ps_place_colliders(")
            < code.index("ps_place_colliders_device(") < code.index("ps_label_air_pockets("))
    between = code[code.index("ps_paint_collider_velocities_device("):code.index("PS_COLLIDER_SHAPE_REACH")]
    assert "typedef" not in between and between.count(";") == 1
    for name in ARRAYS:
        assert '"%s"' % name in hdr, name
    for needle in ("r_m = orig_m + ((double)i_m + 0.5) * dx", "q_a = (R[0][a]*d_0 + R[1][a]*d_1) + R[2][a]*d_2", "s_a = (q_a - o_a) / h - 0.5",
                   "E = (PS_COLLIDER_SHAPE_REACH * dx) / h", "i_a = min((int)floor(c_a), n_a - 2)", "lo + (hi - lo) * f",
                   "dist = sqrt((out_0*out_0 + out_1*out_1) + out_2*out_2)", "D_k = (negate ? -val : val) - dist", "if D_k > D_best",
                   "collision[c] = (float)(negate ? -D_best : D_best)", "counted once in slot count + 1",
                   "count outside 0..64", "shape N: extent outside 2..1022", "shape N: spacing not positive and finite", "shape N: origin not finite",
                   "shape N: no samples", "shape N: non-finite value at sample M", "count differs from the shapes' count",
                   "pose of collider N is not finite", "not 8-byte aligned", "no shapes set",
                   "4 bytes per sample", "96 * count + 4 * (count + 2)", "one int32 cell grid", "ps_memory_stats entry 2 is 0",
                   "never see a placement", "the weights stay the caller's", "does not re-place", "drops the air-pocket labels", "Out of scope"):
        assert needle in hdr, needle
    body = code[code.index("typedef struct ps_params {"):code.index("} ps_params;")]
    assert "hape" not in body and "pose" not in body                                    # calls on a context, not ps_params members


def _typed(lib):
    from polystokes_amd import _abi as abi
    for name, argtypes in abi.COLLIDER_SHAPE_CALLS:
        assert hasattr(lib, name), name
        getattr(lib, name).argtypes = list(argtypes)
        getattr(lib, name).restype = ctypes.c_int32
    return lib


def test_every_library_exports_them_and_refuses_a_null_context():
    import polystokes_amd
    from polystokes_amd import _abi as abi
    assert tuple(n for n, _ in abi.COLLIDER_SHAPE_CALLS) == SYMBOLS
    for sym in SYMBOLS:
        assert sym in polystokes_amd.EXPORTED_SYMBOLS, sym
    L = polystokes_amd.lib()
    libs = [L] + [ctypes.CDLL(os.path.join(ROOT, "polystokes_amd", n)) for n in ("libpolystokes_hip_release.so", "libpolystokes_hip_affine.so")]
    tab = (ctypes.c_double * 12)()
    poses = abi.ColliderPoses(1, ctypes.addressof(tab))
    shapes = abi.ColliderShapes(0, None)
    for lib in libs:
        _typed(lib)
        assert lib.ps_set_collider_shapes(None, ctypes.byref(shapes)) == abi.FAILED
        assert lib.ps_place_colliders(None, ctypes.byref(poses)) == abi.FAILED
        assert lib.ps_place_colliders_device(None, None, 1, None) == abi.FAILED
        lib.ps_abi_version.restype = ctypes.c_int32
        assert lib.ps_abi_version() == 1
    mk = _read("polystokes_amd", "csrc", "Makefile")
    assert re.search(r"^SRC := .*\bps_shapes\.hip\b", mk, flags=re.M)                   # in the one list all three libraries build from
    src = _read("polystokes_amd", "csrc", "ps_shapes.hip")
    assert "getenv" not in src and re.findall(r"PS_ENV\w*\(\"(\w+)\"\)", src) == ["PS_DEBUG_SHAPE_CULL"]       # one test-only switch, lab build only
    assert len(re.findall(r"PS_ENV_LOUD\(", src)) == 1
    assert "PS_DEBUG_SHAPE_CULL" in _read("README.md")
    assert "atomicAdd(&T.cells" in src and not re.search(r"atomicAdd\([^;]*(float|double)", src)              # integer counters only


def test_python_layer_carries_them():
    import numpy as np
    import polystokes_amd
    from polystokes_amd import _abi as abi
    S = abi.ColliderShape
    assert ctypes.sizeof(S) == 56
    assert (S.n.offset, S.reserved.offset, S.h.offset, S.orig.offset, S.sdf.offset) == (0, 12, 16, 24, 48)
    assert ctypes.sizeof(abi.ColliderShapes) == 16 and abi.ColliderShapes.count.offset == 0 and abi.ColliderShapes.shape.offset == 8
    assert ctypes.sizeof(abi.ColliderPoses) == 16 and abi.ColliderPoses.count.offset == 0 and abi.ColliderPoses.pose.offset == 8
    assert abi.COLLIDER_SHAPE_REACH == 4.0
    for name in ("set_collider_shapes", "place_colliders", "place_colliders_device"):
        assert callable(getattr(polystokes_amd.Solver, name)), name
    for name in ("colliderShapes", "colliderPlacement", "colliderPlacedCells", "colliderCellIds"):
        assert polystokes_amd._kind(name) == "i", name
    for name in ("colliderPoseTable", "collisionField"):
        assert polystokes_amd._kind(name) == "f", name
    assert polystokes_amd._DT[(8, "f")] is np.float64 and polystokes_amd._DT[(4, "f")] is np.float32


def test_documents_describe_it():
    readme = _read("README.md")
    assert "ps_set_collider_shapes" in readme and "ps_place_colliders" in readme
    design = _read("DESIGN.md")
    heads = [m.group(1).strip() for m in re.finditer(r"^#+ (.*)$", design, flags=re.M)]
    motions = [i for i, h in enumerate(heads) if "Collider motions" in h]
    shapes = [i for i, h in enumerate(heads) if "Collider shapes" in h]
    assert motions and shapes and shapes[0] == motions[0] + 1                           # the section follows the motions'
    section = design[design.index("Collider shapes"):]
    assert "Out of scope" in section[:section.index("### Air pockets")]
    assert "ps_place_colliders_device" in _read("INTEGRATION.md")
    assert os.path.exists(os.path.join(ROOT, "profiles", "collider_shapes.md"))
    assert os.path.exists(os.path.join(ROOT, "scripts", "collider_shapes_ab.py"))

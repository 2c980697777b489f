"""CPU-side checks of the device-resident field calls (ps_*_device): the ABI surface, the documented contract, and the index rule that
the harness's numpy re-layout and the header's formulas must agree on."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ps_upload_fields_device", "ps_upload_density_field_device", "ps_download_fields_device",
         "ps_download_solution_fields_device", "ps_step_device_fields"]


def _header():
    return open(os.path.join(ROOT, "include", "polystokes.h")).read()


def test_symbols_are_declared_exported_and_listed():
    import polystokes_amd
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint32_t\s+" + n + r"\s*\(", code), n
        assert n in polystokes_amd.EXPORTED_SYMBOLS, n
    for so in ("libpolystokes_hip.so", "libpolystokes_hip_affine.so", "libpolystokes_hip_release.so"):
        L = ctypes.CDLL(os.path.join(ROOT, "polystokes_amd", so))
        for n in NAMES:
            assert hasattr(L, n), (so, n)


def test_layout_constants_match_the_header():
    from polystokes_amd import _abi
    m = re.search(r"enum\s+ps_field_layout\s*\{\s*PS_LAYOUT_X_FASTEST\s*=\s*(\d+)\s*,\s*PS_LAYOUT_Z_FASTEST\s*=\s*(\d+)\s*\}", _header())
    assert m, "enum ps_field_layout"
    assert (_abi.LAYOUT_X_FASTEST, _abi.LAYOUT_Z_FASTEST) == (int(m.group(1)), int(m.group(2))) == (0, 1)


def test_header_documents_layouts_streams_and_refusals():
    txt = " ".join(_header().split())
    for needle in ("i + d0*(j + d1*k)", "k + d2*(j + d1*i)",                                  # the two index rules
                   "hipStream_t", "NULL: the default stream", "never runs its own work on it",   # the stream contract
                   "inputs consumed", "WITHOUT synchronising the host", "may alias in->vel[a]",
                   "a layout other than 0 or 1", "a required field that is null", "not 4-byte aligned",   # the refusals
                   "hipPointerGetAttributes", "pinned host, managed", "other-device memory", "hipMemGetAddressRange",
                   "the context unchanged and usable"):
        assert needle in txt, needle


def test_numpy_relayout_agrees_with_the_header_formulas():
    """device_scene stores np.ascontiguousarray(a.transpose(2, 1, 0)) of a (z, y, x) array for layout 1: entry k + d2*(j + d1*i) of
    that must be entry i + d0*(j + d1*k) of the x-fastest array, for every sample, on a grid with three different extents."""
    import polystokes_amd
    from polystokes_amd import _abi
    d0, d1, d2 = 71, 5, 66
    xf = np.arange(d0 * d1 * d2, dtype=np.float32).reshape(d2, d1, d0)      # (z, y, x), x fastest: the host calls' arrays
    zf = polystokes_amd.to_layout(xf, _abi.LAYOUT_Z_FASTEST)
    assert zf.shape == (d0, d1, d2) and zf.flags["C_CONTIGUOUS"]
    assert np.array_equal(zf, np.ascontiguousarray(xf.transpose(2, 1, 0)))
    i, j, k = np.meshgrid(np.arange(d0), np.arange(d1), np.arange(d2), indexing="ij")
    assert np.array_equal(xf.ravel()[i + d0 * (j + d1 * k)], zf.ravel()[k + d2 * (j + d1 * i)])
    assert polystokes_amd.to_layout(xf, _abi.LAYOUT_X_FASTEST).ravel().tobytes() == xf.tobytes()
    for layout in (0, 1):
        assert np.array_equal(polystokes_amd.from_layout(polystokes_amd.to_layout(xf, layout).ravel(), xf.shape, layout), xf)


def test_device_address_and_stream_forms():
    """The harness takes an int, `.ptr`, `data_ptr()` or `__cuda_array_interface__` for an array and an int or `.cuda_stream` for a stream."""
    import polystokes_amd

    class P:
        ptr = 0x1000

    class T:
        def data_ptr(self):
            return 0x2000

    class A:
        __cuda_array_interface__ = {"data": (0x3000, False)}

    class S:
        cuda_stream = 0x40

    assert [polystokes_amd.device_address(v) for v in (None, 7, P(), T(), A())] == [None, 7, 0x1000, 0x2000, 0x3000]
    assert [polystokes_amd.stream_handle(v) for v in (None, 5, S())] == [None, 5, 0x40]

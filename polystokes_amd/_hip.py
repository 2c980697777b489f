"""ctypes binding of the few HIP runtime calls the harness needs to act as a device-resident caller (tests, scripts; not the product).

The symbols are resolved through the handle of libpolystokes_hip.so, i.e. from the HIP runtime the library itself maps: no second
runtime is loaded and torch is not imported (tests/test_abi_cpu.py::test_no_gpu_fails_loudly says why the harness avoids that)."""
import ctypes as C

import numpy as np

H2D, D2H, D2D = 1, 2, 3     # hipMemcpyKind
_rt = None


class HipError(RuntimeError):
    pass


def rt():
    global _rt
    if _rt is None:
        from . import lib
        L = lib()
        vp, sz = C.c_void_p, C.c_size_t
        sig = {
            "hipMalloc": [C.POINTER(vp), sz], "hipFree": [vp], "hipMemcpy": [vp, vp, sz, C.c_int],
            "hipMemcpyAsync": [vp, vp, sz, C.c_int, vp], "hipHostMalloc": [C.POINTER(vp), sz, C.c_uint], "hipHostFree": [vp],
            "hipStreamCreate": [C.POINTER(vp)], "hipStreamDestroy": [vp], "hipStreamSynchronize": [vp],
        }
        for name, args in sig.items():
            fn = getattr(L, name)
            fn.argtypes, fn.restype = args, C.c_int
        _rt = L
    return _rt


def check(rc, what):
    if rc != 0:
        raise HipError(f"{what} failed with hipError_t {rc}")


def memcpy(dst, src, nbytes, kind):
    check(rt().hipMemcpy(dst, src, nbytes, kind), "hipMemcpy")


def memcpy_async(dst, src, nbytes, kind, stream):
    check(rt().hipMemcpyAsync(dst, src, nbytes, kind, stream), "hipMemcpyAsync")


class Stream:
    """A hipStream_t of the harness; `.cuda_stream` is its address (the attribute torch streams carry)."""

    def __init__(self):
        s = C.c_void_p()
        check(rt().hipStreamCreate(C.byref(s)), "hipStreamCreate")
        self.cuda_stream = s.value

    def synchronize(self):
        check(rt().hipStreamSynchronize(self.cuda_stream), "hipStreamSynchronize")

    def close(self):
        if self.cuda_stream:
            rt().hipStreamDestroy(self.cuda_stream)
            self.cuda_stream = None


class HostBuffer:
    """Page-locked host floats (hipHostMalloc), viewed as a numpy array."""

    def __init__(self, count):
        p = C.c_void_p()
        check(rt().hipHostMalloc(C.byref(p), max(int(count), 1) * 4, 0), "hipHostMalloc")
        self.ptr, self.count = p.value, int(count)
        self.array = np.ctypeslib.as_array(C.cast(self.ptr, C.POINTER(C.c_float)), shape=(max(self.count, 1),))[:self.count]

    def close(self):
        if self.ptr:
            self.array = None
            rt().hipHostFree(self.ptr)
            self.ptr = None


class DeviceBuffer:
    """`count` floats of device memory, `pad` spare floats in front: ptr = allocation + 4 * pad (a view with a storage offset)."""

    def __init__(self, count, pad=0):
        p = C.c_void_p()
        self.count, self.nbytes = int(count), int(count) * 4
        check(rt().hipMalloc(C.byref(p), max(self.nbytes + 4 * pad, 4)), "hipMalloc")
        self.base = p.value
        self.ptr = self.base + 4 * pad

    @classmethod
    def from_numpy(cls, a, pad=0):
        a = np.ascontiguousarray(a, dtype=np.float32)
        b = cls(a.size, pad)
        if a.size:
            memcpy(b.ptr, a.ctypes.data, a.nbytes, H2D)
        return b

    def to_numpy(self, shape=None):
        """A blocking copy on the default stream (which waits for every blocking stream of the process)."""
        out = np.empty(self.count, np.float32)
        if self.count:
            memcpy(out.ctypes.data, self.ptr, self.nbytes, D2H)
        return out if shape is None else out.reshape(shape)

    def close(self):
        if self.base:
            rt().hipFree(self.base)
            self.base = self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

"""Device memory owned from Python: the one handle to the HIP runtime and a small owner class over hipMalloc / hipMemcpy.

The renderer's few buffers of its own (engine.Renderer._device_buffer), the tests and the timing tools all allocate through
here, so that every byte they hand to the library comes from the runtime the library itself uses."""
import ctypes as C

import numpy as np

from . import _capi

_H2D, _D2H = 1, 2   # hipMemcpyHostToDevice, hipMemcpyDeviceToHost

_handle = None


class RtError(RuntimeError):
    pass


def hip():
    """The HIP runtime the library is bound to. Looked up through the library's own handle (dlsym searches a library and then
    its dependencies) and not by the runtime's file name, so that a second copy of the runtime in the process (a framework's
    wheel bundles one) is never taken for it: memory from that copy would be foreign to the library's device context."""
    global _handle
    if _handle is None:
        h = C.CDLL(_capi.LIB_PATH)
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipFree.argtypes = [C.c_void_p]
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        h.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        h.hipDeviceSynchronize.argtypes = []
        _handle = h
    return _handle


def synchronize():
    if hip().hipDeviceSynchronize() != 0:
        raise RtError("hipDeviceSynchronize failed")


class DeviceBuffer:
    """`nbytes` of device memory (at least one byte is allocated, so .ptr is never null). Copies block, are checked against the
    buffer's size, and do nothing for zero bytes. `error=` replaces the message of the RtError a failed copy raises."""

    def __init__(self, nbytes, name=None):
        self.nbytes = int(nbytes)
        q = C.c_void_p()
        if hip().hipMalloc(C.byref(q), max(self.nbytes, 1)) != 0 or not q.value:
            raise RtError(f"no device memory for {self.nbytes} bytes" + (f" ({name})" if name else ""))
        self.ptr = q.value

    def _span(self, n, offset, what):
        if not self.ptr:
            raise RtError(f"{what}: the buffer was freed")
        if offset < 0 or offset + n > self.nbytes:
            raise ValueError(f"{what}: bytes [{offset}, {offset + n}) of a buffer of {self.nbytes}")
        return self.ptr + offset

    def upload(self, array, offset=0, error=None):
        a = np.ascontiguousarray(array)
        d = self._span(a.nbytes, offset, "upload")
        if a.nbytes and hip().hipMemcpy(d, a.ctypes.data, a.nbytes, _H2D) != 0:
            raise RtError(error or f"hipMemcpy of {a.nbytes} bytes to the device failed")
        return self

    def download(self, shape=None, dtype=np.uint8, into=None, offset=0, error=None):
        """A new array of `shape` and `dtype` (all the buffer's bytes by default), or the contiguous array `into`, filled."""
        out = into if into is not None else np.empty((self.nbytes - offset) // np.dtype(dtype).itemsize if shape is None else shape, dtype)
        if not out.flags.c_contiguous:
            raise ValueError("download: `into` is not contiguous")
        d = self._span(out.nbytes, offset, "download")
        if out.nbytes and hip().hipMemcpy(out.ctypes.data, d, out.nbytes, _D2H) != 0:
            raise RtError(error or f"hipMemcpy of {out.nbytes} bytes from the device failed")
        return out

    def fill(self, byte):
        self._span(0, 0, "fill")
        if self.nbytes and hip().hipMemset(self.ptr, int(byte), self.nbytes) != 0:
            raise RtError(f"hipMemset of {self.nbytes} bytes failed")
        return self

    def free(self):
        if getattr(self, "ptr", None) and _handle is not None:   # (None again once the interpreter is shutting down)
            _handle.hipFree(self.ptr)
            self.ptr = None

    __del__ = free

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

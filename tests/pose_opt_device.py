"""Device buffers for the GPU tests on device pointers and tools/pose_opt_timing.py (Dev: a device copy of an array; Out: an output
between guard bytes), through the library's own allocator
(orbfe_device_alloc / _upload_rows / _download: ordinary HIP device pointers of the library's runtime; the download is blocking, so
it also waits for work enqueued on the null stream)."""
import ctypes as C

import numpy as np

from orb_slam2_aruco_amd import binding

_L = None


def _lib():
    global _L
    if _L is None:
        _L = binding.load()
    return _L


class Dev:
    """A device copy of a numpy array (same dtype and shape)."""

    def __init__(self, a):
        L = _lib()
        self.a = np.ascontiguousarray(a)
        self.nbytes = max(self.a.nbytes, 1)
        self.ptr = L.orbfe_device_alloc(0, self.nbytes)
        if not self.ptr:
            raise RuntimeError("orbfe_device_alloc: %s" % L.orbfe_last_error().decode())
        if self.a.nbytes and L.orbfe_device_upload_rows(self.ptr, self.a.nbytes, self.a.ctypes.data_as(C.c_void_p), self.a.nbytes,
                                                        self.a.nbytes, 1) != 0:
            raise RuntimeError("orbfe_device_upload_rows: %s" % L.orbfe_last_error().decode())

    def put(self, a):
        """the same bytes again from another array of this shape and dtype"""
        src = np.ascontiguousarray(a, self.a.dtype).reshape(self.a.shape)
        if src.nbytes and _lib().orbfe_device_upload_rows(self.ptr, src.nbytes, src.ctypes.data_as(C.c_void_p), src.nbytes, src.nbytes, 1) != 0:
            raise RuntimeError("orbfe_device_upload_rows: %s" % _lib().orbfe_last_error().decode())

    def get(self):
        out = np.empty_like(self.a)
        if out.nbytes and _lib().orbfe_device_download(out.ctypes.data_as(C.c_void_p), self.ptr, out.nbytes) != 0:
            raise RuntimeError("orbfe_device_download: %s" % _lib().orbfe_last_error().decode())
        return out

    def __del__(self):
        if getattr(self, "ptr", None) and _L is not None:
            _L.orbfe_device_free(self.ptr)
            self.ptr = None


class Out:
    """A device output with 256 guard bytes in front and behind; get() asserts that both are unchanged."""
    GUARD = 256

    def __init__(self, init):
        self.a = np.ascontiguousarray(init)
        self.dev = Dev(self._raw(self.a))
        self.ptr = self.dev.ptr + self.GUARD

    def _raw(self, a):
        return np.concatenate([np.full(self.GUARD, 0xC3, np.uint8), a.view(np.uint8).reshape(-1), np.full(self.GUARD, 0x3C, np.uint8)])

    def put(self, a):
        """the whole buffer again, guards included"""
        self.dev.put(self._raw(np.ascontiguousarray(a, self.a.dtype).reshape(self.a.shape)))

    def get(self):
        raw = self.dev.get()
        assert np.all(raw[:self.GUARD] == 0xC3), "bytes in front of the output were overwritten"
        assert np.all(raw[-self.GUARD:] == 0x3C), "bytes behind the output were overwritten"
        return raw[self.GUARD:-self.GUARD].view(self.a.dtype).reshape(self.a.shape)

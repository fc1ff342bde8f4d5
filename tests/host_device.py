"""numpy memory in the place of the device, for the CPU tests of the GPU harnesses (tests/test_pfb_gpu_harness_cpu.py,
test_fir_gpu_harness_cpu.py): HOST stands in for smfft_amd (DeviceBuffer, smfft_memset, the copies, smfft_synchronize), and a launch is
a Python function that reads and writes through the pointers it is given.  A plain module: no tests, no fixtures."""
import ctypes
import types

import numpy as np


class HostBuffer:
    def __init__(self, nbytes):
        self.mem, self.nbytes = np.zeros(nbytes, np.uint8), nbytes
        self.ptr = self.mem.ctypes.data

    @classmethod
    def from_host(cls, a):
        b = cls(a.nbytes)
        b.mem[:] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        return b

    def to_host(self, dtype, shape):
        return self.mem.view(dtype).reshape(shape).copy()

    def free(self):
        self.mem = None


def _memset(ptr, byte, nbytes):
    ctypes.memset(ptr, byte, nbytes)
    return 0


def _memcpy(dst, src, nbytes):
    ctypes.memmove(dst, src, nbytes)
    return 0


HOST = types.SimpleNamespace(DeviceBuffer=HostBuffer, lib=types.SimpleNamespace(
    smfft_memset=_memset, smfft_memcpy_h2d=_memcpy, smfft_memcpy_d2h=_memcpy, smfft_synchronize=lambda: 0))


def at(ptr, dtype, n):
    """n elements of dtype at the address ptr; negative indices are not meant: pass ptr - k * itemsize"""
    return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint8)), (n * np.dtype(dtype).itemsize,)).view(dtype)

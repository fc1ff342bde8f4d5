"""ctypes mirror of include/smfft_large.h: batched C2C FFTs of N = 8192 and 16384 in one pass through HBM (libsmfft_large.so).

The library is loaded on first use, so that `import smfft_amd` behaves the same whether it was built or not.  Device pointers are
plain integers; transforms are un-normalised, natural order in and out; timings are ADDED to a running total, as in smfft_amd.api.
There is no CPU fallback: a missing library raises on first call.
"""
import ctypes

import numpy as np

from . import _addon

SIZES = (8192, 16384)

_vp, _i, _dp = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double)
# name -> (restype, argtypes), exactly the declarations of include/smfft_large.h (tests/test_large_cpu.py compares them)
SIGS = {
    "smfft_large_launch": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "smfft_large_benchmark": (_i, [_vp, _vp, _i, _i, _i, _dp]),
    "smfft_large_grid": (_i, [_i]),
}

LIB_PATH, load, lib = _addon.loader("libsmfft_large.so", "SMFFT_LARGE_LIB", __name__, SIGS)
_lib = None


def launch(d_in, d_out, N, nFFTs, inverse=False, stream=0):
    """Enqueue d_out[f] = FFT(d_in[f]), f < nFFTs, on a hipStream_t handle (int; 0 = null stream).  No synchronisation."""
    rc = lib().smfft_large_launch(d_in, d_out, N, nFFTs, int(inverse), stream)
    if rc != 0:
        raise RuntimeError(f"smfft_large_launch(N={N}, nFFTs={nFFTs}) -> {rc}")


def benchmark(d_in, d_out, N, nFFTs, inverse=False):
    """One launch on the null stream, timed with events; synchronous.  Returns (status, elapsed_ms)."""
    t = ctypes.c_double(0.0)
    rc = lib().smfft_large_benchmark(d_in, d_out, N, nFFTs, int(inverse), ctypes.byref(t))
    return rc, t.value


def grid(N):
    """the persistent grid of an N-point launch on the current device (workgroups)"""
    return lib().smfft_large_grid(N)


def c2c(x, inverse=False):
    """x: (nFFTs, N) complex64 host array, N = 8192 or 16384 -> its un-normalised DFTs (inverse: the + sign), through the GPU."""
    from . import api      # the device allocator and copies of libsmfft_amd.so
    x = np.ascontiguousarray(x, dtype=np.complex64)
    nffts, n = x.shape
    if n not in SIZES:
        raise ValueError(f"smfft_amd.large serves N = 8192 and 16384, not {n}")
    din = api.DeviceBuffer.from_host(x)
    dout = api.DeviceBuffer(max(x.nbytes, 8))
    api.lib.smfft_memset(dout.ptr, 0xFF, dout.nbytes)     # NaN pattern: untouched outputs are caught
    rc, _ = benchmark(din.ptr, dout.ptr, n, nffts, inverse)
    if rc != 0:
        raise RuntimeError(f"smfft_large_benchmark(N={n}, nFFTs={nffts}) -> {rc}")
    out = dout.to_host(np.complex64, x.shape)
    for b in (din, dout):
        b.free()
    return out

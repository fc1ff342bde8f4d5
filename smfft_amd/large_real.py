"""ctypes mirror of include/smfft_large_real.h: batched R2C / C2R FFTs of real N = 16384 and 32768 in one pass through HBM
(libsmfft_large_real.so).

The library is loaded on first use, so that `import smfft_amd` behaves the same whether it was built or not.  Device pointers are
plain integers; N is the REAL length; R2C writes N/2 complex values in the packed layout (element 0 = (X[0].re, X[N/2].re)), C2R
reads that layout and writes (N/2) x -- the conventions of smfft_rc_external_benchmark.  Timings are ADDED to a running total, as in
smfft_amd.api.  There is no CPU fallback: a missing library raises on first call.
"""
import ctypes

import numpy as np

from . import _addon

SIZES = (16384, 32768)

_vp, _i, _dp = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double)
# name -> (restype, argtypes), exactly the declarations of include/smfft_large_real.h (tests/test_large_real_cpu.py compares them)
SIGS = {
    "smfft_large_real_launch": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "smfft_large_real_benchmark": (_i, [_vp, _vp, _i, _i, _i, _dp]),
    "smfft_large_real_grid": (_i, [_i]),
}

LIB_PATH, load, lib = _addon.loader("libsmfft_large_real.so", "SMFFT_LARGE_REAL_LIB", __name__, SIGS)
_lib = None


def launch(d_in, d_out, N, nFFTs, inverse=False, stream=0):
    """Enqueue R2C (inverse = False) or C2R of nFFTs real N-point FFTs on a hipStream_t handle (int; 0 = null stream)."""
    rc = lib().smfft_large_real_launch(d_in, d_out, N, nFFTs, int(inverse), stream)
    if rc != 0:
        raise RuntimeError(f"smfft_large_real_launch(N={N}, nFFTs={nFFTs}) -> {rc}")


def benchmark(d_in, d_out, N, nFFTs, inverse=False):
    """One launch on the null stream, timed with events; synchronous.  Returns (status, elapsed_ms)."""
    t = ctypes.c_double(0.0)
    rc = lib().smfft_large_real_benchmark(d_in, d_out, N, nFFTs, int(inverse), ctypes.byref(t))
    return rc, t.value


def grid(N):
    """the persistent grid of a real N-point launch on the current device (workgroups)"""
    return lib().smfft_large_real_grid(N)


def _run(x, out_dtype, out_shape, n, inverse):
    from . import api      # the device allocator and copies of libsmfft_amd.so
    din = api.DeviceBuffer.from_host(x)
    dout = api.DeviceBuffer(max(x.nbytes, 8))
    api.lib.smfft_memset(dout.ptr, 0xFF, dout.nbytes)     # NaN pattern: untouched outputs are caught
    rc, _ = benchmark(din.ptr, dout.ptr, n, x.shape[0], inverse)
    if rc != 0:
        raise RuntimeError(f"smfft_large_real_benchmark(N={n}, nFFTs={x.shape[0]}, inverse={int(inverse)}) -> {rc}")
    out = dout.to_host(out_dtype, out_shape)
    for b in (din, dout):
        b.free()
    return out


def r2c(x):
    """x: (nFFTs, N) float32 host array, N = 16384 or 32768 -> (nFFTs, N/2) complex64 in the packed layout, through the GPU."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    nffts, n = x.shape
    if n not in SIZES:
        raise ValueError(f"smfft_amd.large_real serves N = 16384 and 32768, not {n}")
    return _run(x, np.complex64, (nffts, n // 2), n, False)


def c2r(xp):
    """xp: (nFFTs, N/2) complex64 packed spectra, N = 16384 or 32768 -> (nFFTs, N) float32 = (N/2) x, through the GPU."""
    xp = np.ascontiguousarray(xp, dtype=np.complex64)
    nffts, half = xp.shape
    n = 2 * half
    if n not in SIZES:
        raise ValueError(f"smfft_amd.large_real serves N = 16384 and 32768, not {n}")
    return _run(xp, np.float32, (nffts, n), n, True)

"""ctypes mirror of include/smfft_rowconv_real.h: batched linear convolution or correlation of PAIRS of real rows, a[r] with b[r] for
every r, n_a, n_b >= 1 and n_a + n_b - 1 <= 4096, in one kernel (libsmfft_rowconv_real.so: both rows in the two lanes of one forward
transform, each balanced by a power of two from its own energy, the product of the two recovered spectra and one inverse transform of
M = 256 ... 4096 points, M >= n_a + n_b - 1, on the register engine).  float32 in, float32 out.

    convolve:   y[r, k] = sum_j a[r, j] b[r, k - j]                          = np.convolve(a[r], b[r])
    correlate:  y[r, k] = sum_j a[r, j + k - (n_b - 1)] b[r, j]              = np.correlate(a[r], b[r], 'full')
    window:     out[r, i] = y[r, first + i], 0 <= i < m, first + m <= n_a + n_b - 1

The library is loaded on first use, so that `import smfft_amd` behaves the same whether it was built or not.  Device pointers are
plain integers; there is no plan and nothing to prepare; timings are ADDED to a running total, as in smfft_amd.api.  Complex rows are
smfft_amd.rowconv's.  There is no CPU fallback: a missing library raises on first call.
"""
import ctypes

import numpy as np

from . import _addon

SIZES = (256, 512, 1024, 2048, 4096)      # the inner transform lengths M
MAX_FULL = 4096                           # the largest n_a + n_b - 1

_vp, _i, _ll, _dp = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.POINTER(ctypes.c_double)
_HEAD = [_vp, _vp, _vp, _i, _i, _i, _i, _ll, _i]      # d_a, d_b, d_out, n_a, n_b, first, m, batch, correlate
# name -> (restype, argtypes), exactly the declarations of include/smfft_rowconv_real.h (tests/test_sm_rowconv_real_cpu.py compares them)
SIGS = {
    "smfft_rowconv_real_fft_size": (_i, [_i, _i]),
    "smfft_rowconv_real_launch": (_i, _HEAD + [_vp]),
    "smfft_rowconv_real_launch_tuned": (_i, _HEAD + [_vp, _i]),
    "smfft_rowconv_real_benchmark": (_i, _HEAD + [_dp]),
}

LIB_PATH, load, lib = _addon.loader("libsmfft_rowconv_real.so", "SMFFT_ROWCONV_REAL_LIB", __name__, SIGS)
_lib = None


def _check_lengths(n_a, n_b):
    n_a, n_b = int(n_a), int(n_b)
    if n_a < 1 or n_b < 1 or n_a + n_b - 1 > MAX_FULL:
        raise ValueError(f"smfft_amd.rowconv_real serves n_a, n_b >= 1 with n_a + n_b - 1 <= {MAX_FULL}, not n_a = {n_a}, n_b = {n_b}")
    return n_a, n_b


def _check_window(n_a, n_b, first, m):
    """(first, m) with m = the rest of the full result when None"""
    full = n_a + n_b - 1
    first = int(first)
    m = full - first if m is None else int(m)
    if first < 0 or m < 1 or first + m > full:
        raise ValueError(f"smfft_amd.rowconv_real needs 0 <= first, 1 <= m and first + m <= {full}, not first = {first}, m = {m}")
    return first, m


def fft_size(n_a, n_b):
    """M, the length of the kernel's two transforms: the smallest of 256 ... 4096 with M >= n_a + n_b - 1 (smfft_rowconv_real_fft_size)"""
    return lib().smfft_rowconv_real_fft_size(*_check_lengths(n_a, n_b))


def launch(d_a, d_b, d_out, n_a, n_b, first, m, batch, correlate=False, stream=0):
    """batch convolutions (or correlations) of float32 rows of n_a with rows of n_b elements, elements first ... first + m - 1 of each,
    launch only (no events, no sync); d_a == d_b is allowed, d_out must be neither (smfft_rowconv_real_launch)"""
    rc = lib().smfft_rowconv_real_launch(d_a, d_b, d_out, n_a, n_b, first, m, batch, int(bool(correlate)), stream)
    if rc != 0:
        raise RuntimeError(f"smfft_rowconv_real_launch(n_a={n_a}, n_b={n_b}, first={first}, m={m}, batch={batch}) -> {rc}")


def launch_tuned(d_a, d_b, d_out, n_a, n_b, first, m, batch, grid, correlate=False, stream=0):
    """the same launch on `grid` workgroups (>= 1); the result does not depend on it (smfft_rowconv_real_launch_tuned)"""
    rc = lib().smfft_rowconv_real_launch_tuned(d_a, d_b, d_out, n_a, n_b, first, m, batch, int(bool(correlate)), stream, grid)
    if rc != 0:
        raise RuntimeError(f"smfft_rowconv_real_launch_tuned(n_a={n_a}, n_b={n_b}, first={first}, m={m}, batch={batch}, grid={grid}) -> {rc}")


def benchmark(d_a, d_b, d_out, n_a, n_b, first, m, batch, correlate=False):
    """One launch on the null stream, timed with events; synchronous.  Returns (status, elapsed_ms)."""
    t = ctypes.c_double(0.0)
    rc = lib().smfft_rowconv_real_benchmark(d_a, d_b, d_out, n_a, n_b, first, m, batch, int(bool(correlate)), ctypes.byref(t))
    return rc, t.value


def convolve(a, b, correlate=False, first=0, m=None):
    """a: host array (..., n_a), b: host array (..., n_b) of any real dtype with the same leading axes, n_a + n_b - 1 <= 4096 -> float32
    of shape (..., m): elements first ... first + m - 1 of np.convolve(a[...], b[...]) (or, with correlate,
    np.correlate(a[...], b[...], 'full')) along the last axis, from one fused launch.  m = the rest of the full result by default.
    Complex input raises TypeError: that is smfft_amd.rowconv.convolve"""
    a, b = np.asarray(a), np.asarray(b)
    if np.iscomplexobj(a) or np.iscomplexobj(b):
        raise TypeError("smfft_amd.rowconv_real.convolve takes real rows; complex rows are smfft_amd.rowconv.convolve's")
    if a.ndim < 1 or b.ndim < 1:
        raise ValueError("a and b must have at least one axis")
    if a.shape[:-1] != b.shape[:-1]:
        raise ValueError(f"a and b must pair row by row: leading axes {a.shape[:-1]} and {b.shape[:-1]} differ")
    n_a, n_b = _check_lengths(a.shape[-1], b.shape[-1])                          # (refuses before anything touches a device)
    first, m = _check_window(n_a, n_b, first, m)
    shape = a.shape[:-1] + (m,)
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, n_a)
    b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1, n_b)
    batch = a.shape[0]
    handle = lib()
    from . import api      # the device allocator and the copies of libsmfft_amd.so
    da, db, dout = api.DeviceBuffer.from_host(a), api.DeviceBuffer.from_host(b), api.DeviceBuffer(max(batch * m * 4, 4))
    api.lib.smfft_memset(dout.ptr, 0xFF, dout.nbytes)   # NaN pattern: untouched outputs are caught
    rc = handle.smfft_rowconv_real_launch(da.ptr, db.ptr, dout.ptr, n_a, n_b, first, m, batch, int(bool(correlate)), None)
    if rc == 0:
        rc = api.lib.smfft_synchronize()
    if rc != 0:
        raise RuntimeError(f"rowconv_real.convolve(n_a={n_a}, n_b={n_b}, first={first}, m={m}, batch={batch}) -> {rc}")
    out = dout.to_host(np.float32, (batch, m)).reshape(shape)
    for buf in (da, db, dout):
        buf.free()
    return out

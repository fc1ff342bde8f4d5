"""ctypes mirror of include/smfft_bluestein.h: batched complex-to-complex FFTs of any length 1 <= n <= 2048 in one kernel
(libsmfft_bluestein.so, Bluestein's algorithm on the register engine's transforms of M = 256 ... 4096 points).

The library is loaded on first use, so that `import smfft_amd` behaves the same whether it was built or not.  Device pointers are
plain integers; the plan (2M complex64: the chirp W and the spectrum B) is prepared once per (n, direction) and holds the direction:
the launch takes none; the inverse is un-normalised, as everywhere in smfft_amd; timings are ADDED to a running total, as in
smfft_amd.api.  Powers of two are accepted, but smfft_amd.c2c / smfft_launch serve them more cheaply.  There is no CPU fallback: a
missing library raises on first call.
"""
import ctypes

import numpy as np

from . import _addon

SIZES = (256, 512, 1024, 2048, 4096)      # the inner transform lengths M
MAX_LENGTH = 2048

_vp, _i, _ll, _dp = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.POINTER(ctypes.c_double)
_HEAD = [_vp, _vp, _i, _ll, _vp]      # d_in, d_out, n, batch, d_plan
# name -> (restype, argtypes), exactly the declarations of include/smfft_bluestein.h (tests/test_sm_bluestein_cpu.py compares them)
SIGS = {
    "smfft_bluestein_fft_size": (_i, [_i]),
    "smfft_bluestein_plan_bytes": (_ll, [_i]),
    "smfft_bluestein_tables": (_i, [_i, _i, _vp]),
    "smfft_bluestein_prepare": (_i, [_i, _i, _vp, _vp]),
    "smfft_bluestein_launch": (_i, _HEAD + [_vp]),
    "smfft_bluestein_launch_tuned": (_i, _HEAD + [_vp, _i]),
    "smfft_bluestein_benchmark": (_i, _HEAD + [_dp]),
}

LIB_PATH, load, lib = _addon.loader("libsmfft_bluestein.so", "SMFFT_BLUESTEIN_LIB", __name__, SIGS)
_lib = None


def _check_length(n):
    if not 1 <= int(n) <= MAX_LENGTH:
        raise ValueError(f"smfft_amd.bluestein serves n = 1 ... {MAX_LENGTH}, not n = {n}")
    return int(n)


def fft_size(n):
    """M, the length of the kernel's two transforms: the smallest of 256 ... 4096 with M >= 2n - 1 (smfft_bluestein_fft_size)"""
    return lib().smfft_bluestein_fft_size(_check_length(n))


def plan_bytes(n):
    """bytes of the plan of length n: 16 M (smfft_bluestein_plan_bytes)"""
    return lib().smfft_bluestein_plan_bytes(_check_length(n))


def tables(n, inverse=False):
    """the plan of (n, direction) as the library builds it on the host: (2M,) complex64, W[0, M) then B[0, M) (smfft_bluestein_tables;
    no device is touched)"""
    M = fft_size(n)
    plan = np.empty(2 * M, np.complex64)
    rc = lib().smfft_bluestein_tables(n, int(bool(inverse)), plan.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"smfft_bluestein_tables(n={n}) -> {rc}")
    return plan


def prepare(n, d_plan, inverse=False, stream=0):
    """builds the plan of (n, direction) and copies it to the plan_bytes(n) bytes at d_plan; returns after the copy
    (smfft_bluestein_prepare)"""
    rc = lib().smfft_bluestein_prepare(n, int(bool(inverse)), d_plan, stream)
    if rc != 0:
        raise RuntimeError(f"smfft_bluestein_prepare(n={n}) -> {rc}")


def launch(d_in, d_out, n, batch, d_plan, stream=0):
    """batch transforms of n points in the direction of the prepared plan, launch only (no events, no sync); d_out == d_in is allowed
    (smfft_bluestein_launch)"""
    rc = lib().smfft_bluestein_launch(d_in, d_out, n, batch, d_plan, stream)
    if rc != 0:
        raise RuntimeError(f"smfft_bluestein_launch(n={n}, batch={batch}) -> {rc}")


def launch_tuned(d_in, d_out, n, batch, d_plan, grid, stream=0):
    """the same launch on `grid` workgroups (>= 1); the result does not depend on it (smfft_bluestein_launch_tuned)"""
    rc = lib().smfft_bluestein_launch_tuned(d_in, d_out, n, batch, d_plan, stream, grid)
    if rc != 0:
        raise RuntimeError(f"smfft_bluestein_launch_tuned(n={n}, batch={batch}, grid={grid}) -> {rc}")


def benchmark(d_in, d_out, n, batch, d_plan):
    """One launch on the null stream, timed with events; synchronous.  Returns (status, elapsed_ms)."""
    t = ctypes.c_double(0.0)
    rc = lib().smfft_bluestein_benchmark(d_in, d_out, n, batch, d_plan, ctypes.byref(t))
    return rc, t.value


def fft(x, inverse=False):
    """x: host array (..., n) of any real or complex dtype, 1 <= n <= 2048 -> complex64 of the same shape: the DFT along the last
    axis (np.fft.fft; inverse: np.fft.ifft * n, un-normalised), from one fused launch"""
    x = np.asarray(x)
    if x.ndim < 1:
        raise ValueError("x must have at least one axis")
    n = _check_length(x.shape[-1])         # (refuses before anything touches a device)
    shape = x.shape
    x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1, n)
    batch = x.shape[0]
    handle = lib()
    from . import api      # the device allocator and the copies of libsmfft_amd.so
    din, dout = api.DeviceBuffer.from_host(x), api.DeviceBuffer(max(batch * n * 8, 8))
    dplan = api.DeviceBuffer(handle.smfft_bluestein_plan_bytes(n))
    api.lib.smfft_memset(dout.ptr, 0xFF, dout.nbytes)   # NaN pattern: untouched outputs are caught
    rc = handle.smfft_bluestein_prepare(n, int(bool(inverse)), dplan.ptr, None)
    if rc == 0:
        rc = handle.smfft_bluestein_launch(din.ptr, dout.ptr, n, batch, dplan.ptr, None)
    if rc == 0:
        rc = api.lib.smfft_synchronize()
    if rc != 0:
        raise RuntimeError(f"bluestein.fft(n={n}, batch={batch}, inverse={bool(inverse)}) -> {rc}")
    out = dout.to_host(np.complex64, (batch, n)).reshape(shape)
    for b in (din, dout, dplan):
        b.free()
    return out

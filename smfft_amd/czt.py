"""ctypes mirror of include/smfft_czt.h: batched chirp-z (zoom) transforms, m spectral points on an arc of the unit circle from rows of
n samples, 1 <= n, m <= 2048, in one kernel (libsmfft_czt.so, Bluestein's algorithm on the register engine's transforms of
M = 256 ... 4096 points, M >= n + m - 1).

    out[r, k] = sum_j in[r, j] exp(-2 pi i j (start + k step)),  0 <= k < m      (start, step in cycles per sample; un-normalised)

The library is loaded on first use, so that `import smfft_amd` behaves the same whether it was built or not.  Device pointers are
plain integers; the plan (3M complex64: the input chirp A, the spectrum B, the output chirp C) is prepared once per
(n, m, start, step) and holds the arc and the direction: the launch takes neither; timings are ADDED to a running total, as in
smfft_amd.api.  start = 0, step = 1 / n, m = n is the DFT, which smfft_amd.bluestein (any n) and smfft_amd.c2c (powers of two) serve
more cheaply.  There is no CPU fallback: a missing library raises on first call.
"""
import ctypes
import math

import numpy as np

from . import _addon

SIZES = (256, 512, 1024, 2048, 4096)      # the inner transform lengths M
MAX_LENGTH = 2048

_vp, _i, _ll, _d, _dp = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double, ctypes.POINTER(ctypes.c_double)
_HEAD = [_vp, _vp, _i, _i, _ll, _vp]      # d_in, d_out, n, m, batch, d_plan
# name -> (restype, argtypes), exactly the declarations of include/smfft_czt.h (tests/test_sm_czt_cpu.py compares them)
SIGS = {
    "smfft_czt_fft_size": (_i, [_i, _i]),
    "smfft_czt_plan_bytes": (_ll, [_i, _i]),
    "smfft_czt_tables": (_i, [_i, _i, _d, _d, _vp]),
    "smfft_czt_prepare": (_i, [_i, _i, _d, _d, _vp, _vp]),
    "smfft_czt_launch": (_i, _HEAD + [_vp]),
    "smfft_czt_launch_tuned": (_i, _HEAD + [_vp, _i]),
    "smfft_czt_benchmark": (_i, _HEAD + [_dp]),
}

LIB_PATH, load, lib = _addon.loader("libsmfft_czt.so", "SMFFT_CZT_LIB", __name__, SIGS)
_lib = None


def _check_lengths(n, m):
    for name, v in (("n", n), ("m", m)):
        if not 1 <= int(v) <= MAX_LENGTH:
            raise ValueError(f"smfft_amd.czt serves n, m = 1 ... {MAX_LENGTH}, not {name} = {v}")
    return int(n), int(m)


def _check_arc(start, step):
    start, step = float(start), float(step)
    if not (math.isfinite(start) and math.isfinite(step)):
        raise ValueError(f"smfft_amd.czt needs a finite start and step, not start = {start}, step = {step}")
    return start, step


def fft_size(n, m):
    """M, the length of the kernel's two transforms: the smallest of 256 ... 4096 with M >= n + m - 1 (smfft_czt_fft_size)"""
    return lib().smfft_czt_fft_size(*_check_lengths(n, m))


def plan_bytes(n, m):
    """bytes of the plan of (n, m): 24 M (smfft_czt_plan_bytes)"""
    return lib().smfft_czt_plan_bytes(*_check_lengths(n, m))


def tables(n, m, start, step):
    """the plan of (n, m, start, step) as the library builds it on the host: (3M,) complex64, A[0, M), B[0, M), C[0, M)
    (smfft_czt_tables; no device is touched)"""
    M = fft_size(n, m)
    start, step = _check_arc(start, step)
    plan = np.empty(3 * M, np.complex64)
    rc = lib().smfft_czt_tables(n, m, start, step, plan.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"smfft_czt_tables(n={n}, m={m}) -> {rc}")
    return plan


def prepare(n, m, start, step, d_plan, stream=0):
    """builds the plan of (n, m, start, step) and copies it to the plan_bytes(n, m) bytes at d_plan; returns after the copy
    (smfft_czt_prepare)"""
    rc = lib().smfft_czt_prepare(n, m, start, step, d_plan, stream)
    if rc != 0:
        raise RuntimeError(f"smfft_czt_prepare(n={n}, m={m}, start={start}, step={step}) -> {rc}")


def launch(d_in, d_out, n, m, batch, d_plan, stream=0):
    """batch transforms of n samples to the m points of the prepared plan, launch only (no events, no sync); d_out == d_in is allowed
    only with m == n (smfft_czt_launch)"""
    rc = lib().smfft_czt_launch(d_in, d_out, n, m, batch, d_plan, stream)
    if rc != 0:
        raise RuntimeError(f"smfft_czt_launch(n={n}, m={m}, batch={batch}) -> {rc}")


def launch_tuned(d_in, d_out, n, m, batch, d_plan, grid, stream=0):
    """the same launch on `grid` workgroups (>= 1); the result does not depend on it (smfft_czt_launch_tuned)"""
    rc = lib().smfft_czt_launch_tuned(d_in, d_out, n, m, batch, d_plan, stream, grid)
    if rc != 0:
        raise RuntimeError(f"smfft_czt_launch_tuned(n={n}, m={m}, batch={batch}, grid={grid}) -> {rc}")


def benchmark(d_in, d_out, n, m, batch, d_plan):
    """One launch on the null stream, timed with events; synchronous.  Returns (status, elapsed_ms)."""
    t = ctypes.c_double(0.0)
    rc = lib().smfft_czt_benchmark(d_in, d_out, n, m, batch, d_plan, ctypes.byref(t))
    return rc, t.value


def czt(x, m=None, start=0.0, step=None):
    """x: host array (..., n) of any real or complex dtype, 1 <= n <= 2048 -> complex64 of shape (..., m): the m points
    sum_j x[..., j] exp(-2 pi i j (start + k step)) along the last axis, from one fused launch.  m = n and step = 1 / n by default,
    which with start = 0 is np.fft.fft"""
    x = np.asarray(x)
    if x.ndim < 1:
        raise ValueError("x must have at least one axis")
    n, m = _check_lengths(x.shape[-1], x.shape[-1] if m is None else m)         # (refuses before anything touches a device)
    start, step = _check_arc(start, 1.0 / n if step is None else step)
    shape = x.shape[:-1] + (m,)
    x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1, n)
    batch = x.shape[0]
    handle = lib()
    from . import api      # the device allocator and the copies of libsmfft_amd.so
    din, dout = api.DeviceBuffer.from_host(x), api.DeviceBuffer(max(batch * m * 8, 8))
    dplan = api.DeviceBuffer(handle.smfft_czt_plan_bytes(n, m))
    api.lib.smfft_memset(dout.ptr, 0xFF, dout.nbytes)   # NaN pattern: untouched outputs are caught
    rc = handle.smfft_czt_prepare(n, m, start, step, dplan.ptr, None)
    if rc == 0:
        rc = handle.smfft_czt_launch(din.ptr, dout.ptr, n, m, batch, dplan.ptr, None)
    if rc == 0:
        rc = api.lib.smfft_synchronize()
    if rc != 0:
        raise RuntimeError(f"czt.czt(n={n}, m={m}, batch={batch}, start={start}, step={step}) -> {rc}")
    out = dout.to_host(np.complex64, (batch, m)).reshape(shape)
    for b in (din, dout, dplan):
        b.free()
    return out

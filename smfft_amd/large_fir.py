"""ctypes mirror of include/smfft_large_fir.h: overlap-save FIR filter banks with segments of N = 8192 and 16384, for filters of up to
16383 taps (libsmfft_large_fir.so).

The library is loaded on first use, so that `import smfft_amd` behaves the same whether it was built or not.  Device pointers are
plain integers; the semantics, layouts and spectra format are those of smfft_amd.fir_prepare / fir_launch; timings are ADDED to a
running total, as in smfft_amd.api.  There is no CPU fallback: a missing library raises on first call.
"""
import ctypes

import numpy as np

from . import _addon

SIZES = (8192, 16384)

_vp, _i, _ll, _dp = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.POINTER(ctypes.c_double)
# name -> (restype, argtypes), exactly the declarations of include/smfft_large_fir.h (tests/test_large_fir_cpu.py compares them)
SIGS = {
    "smfft_large_fir_prepare": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "smfft_large_fir_launch": (_i, [_vp, _ll, _i, _vp, _i, _i, _i, _i, _vp, _vp]),
    "smfft_large_fir_benchmark": (_i, [_vp, _ll, _i, _vp, _i, _i, _i, _i, _vp, _dp]),
}

LIB_PATH, load, lib = _addon.loader("libsmfft_large_fir.so", "SMFFT_LARGE_FIR_LIB", __name__, SIGS)
_lib = None


def _mode(mode):
    if mode not in ("convolve", "correlate"):
        raise ValueError(f"mode must be 'convolve' or 'correlate', not {mode!r}")
    return int(mode == "correlate")


def prepare(d_taps, d_spectra, n_taps, n_filters, N, mode="convolve", stream=0):
    """Filter spectra for launch, launch only: d_spectra[k*N + j] = DFT_N(pad_N(g_k))[j] / N, g_k = h_k (convolve) or conj(h_k[::-1])
    (correlate), from d_taps = n_filters x n_taps complex64 (smfft_large_fir_prepare)."""
    rc = lib().smfft_large_fir_prepare(d_taps, n_taps, n_filters, N, _mode(mode), d_spectra, stream)
    if rc != 0:
        raise RuntimeError(f"smfft_large_fir_prepare(M={n_taps}, K={n_filters}, N={N}) -> {rc}")


def launch(d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, d_output, mode="convolve", stream=0):
    """Overlap-save filter bank, launch only (no events, no sync): d_output[(c*K + k)*L + n] = np.convolve(x_c, h_k)[n] (convolve) or
    np.correlate(np.r_[x_c, zeros(M-1)], h_k, 'valid')[n] (correlate), with spectra of prepare in the same mode (smfft_large_fir_launch)."""
    rc = lib().smfft_large_fir_launch(d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, _mode(mode), d_output, stream)
    if rc != 0:
        raise RuntimeError(f"smfft_large_fir_launch(L={L}, C={n_channels}, K={n_filters}, M={n_taps}, N={N}) -> {rc}")


def benchmark(d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, d_output, mode="convolve"):
    """One launch on the null stream, timed with events; synchronous.  Returns (status, elapsed_ms)."""
    t = ctypes.c_double(0.0)
    rc = lib().smfft_large_fir_benchmark(d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, _mode(mode), d_output, ctypes.byref(t))
    return rc, t.value


def fir_fft_size(n_taps):
    """The transform length fir() picks for n_taps taps: the next power of two >= 4 M (the rule of smfft_amd.fir_fft_size), clamped to
    8192 ... 16384."""
    if not 1 <= n_taps < 16384:
        raise ValueError(f"n_taps = {n_taps}: the large filter banks take 1 ... 16383 taps")
    return min(16384, max(8192, 1 << (4 * n_taps - 1).bit_length()))


def fir(x, taps, mode="convolve", fft_size=None):
    """x: (C, L) or (L,) signal, taps: (K, M) or (M,) filters (host arrays; real ones are cast to complex64) -> (C, K, L) complex64:
    out[c, k] = np.convolve(x[c], taps[k])[:L] (mode="convolve") or np.correlate(np.r_[x[c], zeros(M-1)], taps[k], 'valid')
    (mode="correlate"), through the overlap-save kernel with N = fft_size (None: fir_fft_size(M))."""
    corr = _mode(mode)
    x, taps = np.asarray(x), np.asarray(taps)
    if x.ndim not in (1, 2) or taps.ndim not in (1, 2):
        raise ValueError("x must be (C, L) or (L,), taps (K, M) or (M,)")
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.complex64)
    taps = np.ascontiguousarray(np.atleast_2d(taps), dtype=np.complex64)
    (C, L), (K, M) = x.shape, taps.shape
    N = fir_fft_size(M) if fft_size is None else int(fft_size)      # (refuses M >= 16384 before anything touches a device)
    if N not in SIZES or not 1 <= M < N:
        raise ValueError(f"smfft_amd.large_fir serves N = 8192 and 16384 with 1 <= M < N, not N = {N}, M = {M}")
    from . import api      # the device allocator and copies of libsmfft_amd.so
    din, dtaps = api.DeviceBuffer.from_host(x), api.DeviceBuffer.from_host(taps)
    dspec = api.DeviceBuffer(max(K * N * 8, 8))
    dout = api.DeviceBuffer(max(C * K * L * 8, 8))
    api.lib.smfft_memset(dout.ptr, 0xFF, dout.nbytes)   # NaN pattern: untouched outputs are caught
    rc = lib().smfft_large_fir_prepare(dtaps.ptr, M, K, N, corr, dspec.ptr, None)
    if rc == 0:
        rc = lib().smfft_large_fir_launch(din.ptr, L, C, dspec.ptr, K, M, N, corr, dout.ptr, None)
    if rc == 0:
        rc = api.lib.smfft_synchronize()
    if rc != 0:
        raise RuntimeError(f"large_fir.fir(C={C}, L={L}, K={K}, M={M}, N={N}, {mode}) -> {rc}")
    out = dout.to_host(np.complex64, (C, K, L))
    for b in (din, dtaps, dspec, dout):
        b.free()
    return out

"""ctypes mirror of include/smfft_fir_real.h: overlap-save FIR filter banks for real signals and real taps, with segments of
N = 256 ... 4096 (libsmfft_fir_real.so).

The library is loaded on first use, so that `import smfft_amd` behaves the same whether it was built or not.  Device pointers are
plain integers; the semantics and the spectra format are those of smfft_amd.fir_prepare / fir_launch on float32 signals, taps and
outputs; timings are ADDED to a running total, as in smfft_amd.api.  There is no CPU fallback: a missing library raises on first call.
"""
import ctypes

import numpy as np

from . import _addon

SIZES = (256, 512, 1024, 2048, 4096)

_vp, _i, _ll, _dp = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.POINTER(ctypes.c_double)
# name -> (restype, argtypes), exactly the declarations of include/smfft_fir_real.h (tests/test_fir_real_cpu.py compares them)
SIGS = {
    "smfft_fir_real_prepare": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "smfft_fir_real_launch": (_i, [_vp, _ll, _i, _vp, _i, _i, _i, _i, _vp, _vp]),
    "smfft_fir_real_benchmark": (_i, [_vp, _ll, _i, _vp, _i, _i, _i, _i, _vp, _dp]),
}

LIB_PATH, load, lib = _addon.loader("libsmfft_fir_real.so", "SMFFT_FIR_REAL_LIB", __name__, SIGS)
_lib = None


def _mode(mode):
    if mode not in ("convolve", "correlate"):
        raise ValueError(f"mode must be 'convolve' or 'correlate', not {mode!r}")
    return int(mode == "correlate")


def prepare(d_taps, d_spectra, n_taps, n_filters, N, mode="convolve", stream=0):
    """Filter spectra for launch, launch only: d_spectra[k*N + j] = DFT_N(pad_N(g_k))[j] / N, g_k = h_k (convolve) or h_k[::-1]
    (correlate), from d_taps = n_filters x n_taps float32 (smfft_fir_real_prepare)."""
    rc = lib().smfft_fir_real_prepare(d_taps, n_taps, n_filters, N, _mode(mode), d_spectra, stream)
    if rc != 0:
        raise RuntimeError(f"smfft_fir_real_prepare(M={n_taps}, K={n_filters}, N={N}) -> {rc}")


def launch(d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, d_output, mode="convolve", stream=0):
    """Overlap-save filter bank on float32, launch only (no events, no sync): d_output[(c*K + k)*L + n] = np.convolve(x_c, h_k)[n]
    (convolve) or np.correlate(np.r_[x_c, zeros(M-1)], h_k, 'valid')[n] (correlate), with spectra of prepare (or of
    smfft_amd.fir_prepare on the cast taps) in the same mode (smfft_fir_real_launch)."""
    rc = lib().smfft_fir_real_launch(d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, _mode(mode), d_output, stream)
    if rc != 0:
        raise RuntimeError(f"smfft_fir_real_launch(L={L}, C={n_channels}, K={n_filters}, M={n_taps}, N={N}) -> {rc}")


def benchmark(d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, d_output, mode="convolve"):
    """One launch on the null stream, timed with events; synchronous.  Returns (status, elapsed_ms)."""
    t = ctypes.c_double(0.0)
    rc = lib().smfft_fir_real_benchmark(d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, _mode(mode), d_output, ctypes.byref(t))
    return rc, t.value


def fir_fft_size(n_taps):
    """The transform length fir() picks for n_taps taps: the next power of two >= 4 M, clamped to 256 ... 4096 (the rule of
    smfft_amd.fir_fft_size)."""
    if not 1 <= n_taps < 4096:
        raise ValueError(f"n_taps = {n_taps}: the real filter banks take 1 ... 4095 taps")
    return min(4096, max(256, 1 << (4 * n_taps - 1).bit_length()))


def fir(x, taps, mode="convolve", fft_size=None):
    """x: (C, L) or (L,) real signal, taps: (K, M) or (M,) real filters (host arrays, cast to float32) -> (C, K, L) float32:
    out[c, k] = np.convolve(x[c], taps[k])[:L] (mode="convolve") or np.correlate(np.r_[x[c], zeros(M-1)], taps[k], 'valid')
    (mode="correlate"), through the overlap-save kernel with N = fft_size (None: fir_fft_size(M)).  Complex input raises TypeError:
    nothing drops an imaginary part (complex data: smfft_amd.fir)."""
    corr = _mode(mode)
    x, taps = np.asarray(x), np.asarray(taps)
    if np.iscomplexobj(x) or np.iscomplexobj(taps):
        raise TypeError("smfft_amd.fir_real.fir takes real signals and real taps; smfft_amd.fir serves complex ones")
    if x.ndim not in (1, 2) or taps.ndim not in (1, 2):
        raise ValueError("x must be (C, L) or (L,), taps (K, M) or (M,)")
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float32)
    taps = np.ascontiguousarray(np.atleast_2d(taps), dtype=np.float32)
    (C, L), (K, M) = x.shape, taps.shape
    N = fir_fft_size(M) if fft_size is None else int(fft_size)      # (refuses M >= 4096 before anything touches a device)
    if N not in SIZES or not 1 <= M < N:
        raise ValueError(f"smfft_amd.fir_real serves N = 256 ... 4096 with 1 <= M < N, not N = {N}, M = {M}")
    from . import api      # the device allocator and copies of libsmfft_amd.so
    din, dtaps = api.DeviceBuffer.from_host(x), api.DeviceBuffer.from_host(taps)
    dspec = api.DeviceBuffer(max(K * N * 8, 8))
    dout = api.DeviceBuffer(max(C * K * L * 4, 8))
    api.lib.smfft_memset(dout.ptr, 0xFF, dout.nbytes)   # NaN pattern: untouched outputs are caught
    rc = lib().smfft_fir_real_prepare(dtaps.ptr, M, K, N, corr, dspec.ptr, None)
    if rc == 0:
        rc = lib().smfft_fir_real_launch(din.ptr, L, C, dspec.ptr, K, M, N, corr, dout.ptr, None)
    if rc == 0:
        rc = api.lib.smfft_synchronize()
    if rc != 0:
        raise RuntimeError(f"fir_real.fir(C={C}, L={L}, K={K}, M={M}, N={N}, {mode}) -> {rc}")
    out = dout.to_host(np.float32, (C, K, L))
    for b in (din, dtaps, dspec, dout):
        b.free()
    return out

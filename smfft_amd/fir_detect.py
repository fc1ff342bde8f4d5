"""ctypes mirror of include/smfft_fir_detect.h: the detected outputs of the overlap-save FIR filter banks for complex signals and
complex taps, with segments of N = 256 ... 4096 (libsmfft_fir_detect.so): the power |y|^2 of every filter, or per output sample the
largest power over the filters and the filter that gave it.

The library is loaded on first use, so that `import smfft_amd` behaves the same whether it was built or not.  Device pointers are
plain integers; y, the modes and the spectra are those of smfft_amd.fir_prepare / fir_launch (there is no prepare here: the spectra come
from smfft_amd.fir_prepare in the same mode); timings are ADDED to a running total, as in smfft_amd.api.  There is no CPU fallback: a
missing library raises on first call.
"""
import ctypes

import numpy as np

from . import _addon, _fir_bank

SIZES = (256, 512, 1024, 2048, 4096)

_vp, _i, _ll, _dp = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.POINTER(ctypes.c_double)
_HEAD = [_vp, _ll, _i, _vp, _i, _i, _i, _i]      # d_signal, signal_length, n_channels, d_spectra, n_filters, n_taps, FFT_size, correlate
# name -> (restype, argtypes), exactly the declarations of include/smfft_fir_detect.h (tests/test_fir_detect_cpu.py compares them)
SIGS = {
    "smfft_fir_power_launch": (_i, _HEAD + [_vp, _vp]),
    "smfft_fir_power_benchmark": (_i, _HEAD + [_vp, _dp]),
    "smfft_fir_peak_launch": (_i, _HEAD + [_vp, _vp, _vp]),
    "smfft_fir_peak_benchmark": (_i, _HEAD + [_vp, _vp, _dp]),
}

LIB_PATH, load, lib = _addon.loader("libsmfft_fir_detect.so", "SMFFT_FIR_DETECT_LIB", __name__, SIGS)
_lib = None


def _launch(name, d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, outputs, mode, stream):
    rc = getattr(lib(), name)(d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, _fir_bank.mode_flag(mode), *outputs, stream)
    if rc != 0:
        raise RuntimeError(f"{name}(L={L}, C={n_channels}, K={n_filters}, M={n_taps}, N={N}) -> {rc}")


def _benchmark(name, d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, outputs, mode):
    t = ctypes.c_double(0.0)
    rc = getattr(lib(), name)(d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, _fir_bank.mode_flag(mode), *outputs, ctypes.byref(t))
    return rc, t.value


def power_launch(d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, d_power, mode="convolve", stream=0):
    """Detected filter bank, launch only (no events, no sync): d_power[(c*K + k)*L + n] = |y_{c,k}[n]|^2 (float32), y what
    smfft_amd.fir_launch writes with the same spectra (of smfft_amd.fir_prepare) in the same mode (smfft_fir_power_launch)."""
    _launch("smfft_fir_power_launch", d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, (d_power,), mode, stream)


def peak_launch(d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, d_peak, d_index, mode="convolve", stream=0):
    """Best filter per sample, launch only: d_peak[c*L + n] = max_k |y_{c,k}[n]|^2 (float32) and d_index[c*L + n] = the lowest k that
    attains it (int32); a NaN power beats every number and the first NaN wins, as np.max / np.argmax (smfft_fir_peak_launch)."""
    _launch("smfft_fir_peak_launch", d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, (d_peak, d_index), mode, stream)


def power_benchmark(d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, d_power, mode="convolve"):
    """One power launch on the null stream, timed with events; synchronous.  Returns (status, elapsed_ms)."""
    return _benchmark("smfft_fir_power_benchmark", d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, (d_power,), mode)


def peak_benchmark(d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, d_peak, d_index, mode="convolve"):
    """One peak launch on the null stream, timed with events; synchronous.  Returns (status, elapsed_ms)."""
    return _benchmark("smfft_fir_peak_benchmark", d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, (d_peak, d_index), mode)


def _round_trip(what, x, taps, mode, fft_size, outputs, call):
    """host arrays through smfft_amd.fir_prepare and one launch: validates x ((C, L) or (L,)) and taps ((K, M) or (M,)), casts them to
    complex64 and copies them in, fills the outputs of outputs(C, K, L) = [(dtype, shape), ...], prefilled with 0xFF, waits and copies
    them back"""
    corr = _fir_bank.mode_flag(mode)
    x, taps = np.asarray(x), np.asarray(taps)
    if x.ndim not in (1, 2) or taps.ndim not in (1, 2):
        raise ValueError("x must be (C, L) or (L,), taps (K, M) or (M,)")
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.complex64)
    taps = np.ascontiguousarray(np.atleast_2d(taps), dtype=np.complex64)
    (C, L), (K, M) = x.shape, taps.shape
    from . import api      # the device allocator, the copies and the prepare of libsmfft_amd.so
    N = api.fir_fft_size(M) if fft_size is None else int(fft_size)      # (refuses M past the longest length before anything touches a device)
    if N not in SIZES or not 1 <= M < N:
        raise ValueError(f"smfft_amd.fir_detect serves N = {SIZES[0]} ... {SIZES[-1]} with 1 <= M < N, not N = {N}, M = {M}")
    handle = lib()
    din, dtaps = api.DeviceBuffer.from_host(x), api.DeviceBuffer.from_host(taps)
    dspec = api.DeviceBuffer(max(K * N * 8, 8))
    spec = outputs(C, K, L)
    douts = [api.DeviceBuffer(max(int(np.prod(shape)) * np.dtype(dtype).itemsize, 8)) for dtype, shape in spec]
    for d in douts:
        api.lib.smfft_memset(d.ptr, 0xFF, d.nbytes)   # NaN / -1 pattern: untouched outputs are caught
    rc = api.lib.smfft_fir_prepare(dtaps.ptr, M, K, N, corr, dspec.ptr, None)
    if rc == 0:
        rc = call(handle)(din.ptr, L, C, dspec.ptr, K, M, N, corr, *[d.ptr for d in douts], None)
    if rc == 0:
        rc = api.lib.smfft_synchronize()
    if rc != 0:
        raise RuntimeError(f"fir_detect.{what}(C={C}, L={L}, K={K}, M={M}, N={N}, {mode}) -> {rc}")
    outs = [d.to_host(dtype, shape) for d, (dtype, shape) in zip(douts, spec)]
    for b in [din, dtaps, dspec] + douts:
        b.free()
    return outs


def power(x, taps, mode="convolve", fft_size=None):
    """x: (C, L) or (L,) signal, taps: (K, M) or (M,) filters (host arrays, cast to complex64) -> (C, K, L) float32:
    out[c, k] = |smfft_amd.fir(x, taps, mode, fft_size)[c, k]|^2, from one fused launch with N = fft_size (None:
    smfft_amd.fir_fft_size(M), the next power of two >= 4 M, clamped to 256 ... 4096)."""
    return _round_trip("power", x, taps, mode, fft_size, lambda C, K, L: [(np.float32, (C, K, L))], lambda h: h.smfft_fir_power_launch)[0]


def peak(x, taps, mode="convolve", fft_size=None):
    """x, taps as for power -> ((C, L) float32, (C, L) int32): the largest power over the filters per output sample and the lowest
    filter index that attains it (np.max / np.argmax of power(...) along the filter axis, NaN included), from one fused launch."""
    best, index = _round_trip("peak", x, taps, mode, fft_size, lambda C, K, L: [(np.float32, (C, L)), (np.int32, (C, L))],
                              lambda h: h.smfft_fir_peak_launch)
    return best, index

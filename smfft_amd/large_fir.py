"""ctypes mirror of include/smfft_large_fir.h: overlap-save FIR filter banks with segments of N = 8192 and 16384, for filters of up to
16383 taps (libsmfft_large_fir.so).

The library is loaded on first use, so that `import smfft_amd` behaves the same whether it was built or not.  Device pointers are
plain integers; the semantics, layouts and spectra format are those of smfft_amd.fir_prepare / fir_launch; timings are ADDED to a
running total, as in smfft_amd.api.  There is no CPU fallback: a missing library raises on first call.
"""
from . import _addon, _fir_bank

SIZES = (8192, 16384)

# name -> (restype, argtypes), exactly the declarations of include/smfft_large_fir.h (tests/test_large_fir_cpu.py compares them)
SIGS = _fir_bank.sigs("smfft_large_fir")

LIB_PATH, load, lib = _addon.loader("libsmfft_large_fir.so", "SMFFT_LARGE_FIR_LIB", __name__, SIGS)
_lib = None
_bank = _fir_bank.Bank("large_fir", "smfft_large_fir", lib, SIZES, real=False, kind="large ")


def prepare(d_taps, d_spectra, n_taps, n_filters, N, mode="convolve", stream=0):
    """Filter spectra for launch, launch only: d_spectra[k*N + j] = DFT_N(pad_N(g_k))[j] / N, g_k = h_k (convolve) or conj(h_k[::-1])
    (correlate), from d_taps = n_filters x n_taps complex64 (smfft_large_fir_prepare)."""
    _bank.prepare(d_taps, d_spectra, n_taps, n_filters, N, mode, stream)


def launch(d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, d_output, mode="convolve", stream=0):
    """Overlap-save filter bank, launch only (no events, no sync): d_output[(c*K + k)*L + n] = np.convolve(x_c, h_k)[n] (convolve) or
    np.correlate(np.r_[x_c, zeros(M-1)], h_k, 'valid')[n] (correlate), with spectra of prepare in the same mode (smfft_large_fir_launch)."""
    _bank.launch(d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, d_output, mode, stream)


def benchmark(d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, d_output, mode="convolve"):
    """One launch on the null stream, timed with events; synchronous.  Returns (status, elapsed_ms)."""
    return _bank.benchmark(d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, d_output, mode)


def fir_fft_size(n_taps):
    """The transform length fir() picks for n_taps taps: the next power of two >= 4 M (the rule of smfft_amd.fir_fft_size), clamped to
    8192 ... 16384."""
    return _bank.fir_fft_size(n_taps)


def fir(x, taps, mode="convolve", fft_size=None):
    """x: (C, L) or (L,) signal, taps: (K, M) or (M,) filters (host arrays; real ones are cast to complex64) -> (C, K, L) complex64:
    out[c, k] = np.convolve(x[c], taps[k])[:L] (mode="convolve") or np.correlate(np.r_[x[c], zeros(M-1)], taps[k], 'valid')
    (mode="correlate"), through the overlap-save kernel with N = fft_size (None: fir_fft_size(M))."""
    return _bank.fir(x, taps, mode, fft_size)

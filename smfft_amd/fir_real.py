"""ctypes mirror of include/smfft_fir_real.h: overlap-save FIR filter banks for real signals and real taps, with segments of
N = 256 ... 4096 (libsmfft_fir_real.so).

The library is loaded on first use, so that `import smfft_amd` behaves the same whether it was built or not.  Device pointers are
plain integers; the semantics and the spectra format are those of smfft_amd.fir_prepare / fir_launch on float32 signals, taps and
outputs; timings are ADDED to a running total, as in smfft_amd.api.  There is no CPU fallback: a missing library raises on first call.
"""
from . import _addon, _fir_bank

SIZES = (256, 512, 1024, 2048, 4096)

# name -> (restype, argtypes), exactly the declarations of include/smfft_fir_real.h (tests/test_fir_real_cpu.py compares them)
SIGS = _fir_bank.sigs("smfft_fir_real")

LIB_PATH, load, lib = _addon.loader("libsmfft_fir_real.so", "SMFFT_FIR_REAL_LIB", __name__, SIGS)
_lib = None
_bank = _fir_bank.Bank("fir_real", "smfft_fir_real", lib, SIZES, real=True, kind="real ")


def prepare(d_taps, d_spectra, n_taps, n_filters, N, mode="convolve", stream=0):
    """Filter spectra for launch, launch only: d_spectra[k*N + j] = DFT_N(pad_N(g_k))[j] / N, g_k = h_k (convolve) or h_k[::-1]
    (correlate), from d_taps = n_filters x n_taps float32 (smfft_fir_real_prepare)."""
    _bank.prepare(d_taps, d_spectra, n_taps, n_filters, N, mode, stream)


def launch(d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, d_output, mode="convolve", stream=0):
    """Overlap-save filter bank on float32, launch only (no events, no sync): d_output[(c*K + k)*L + n] = np.convolve(x_c, h_k)[n]
    (convolve) or np.correlate(np.r_[x_c, zeros(M-1)], h_k, 'valid')[n] (correlate), with spectra of prepare (or of
    smfft_amd.fir_prepare on the cast taps) in the same mode (smfft_fir_real_launch)."""
    _bank.launch(d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, d_output, mode, stream)


def benchmark(d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, d_output, mode="convolve"):
    """One launch on the null stream, timed with events; synchronous.  Returns (status, elapsed_ms)."""
    return _bank.benchmark(d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, d_output, mode)


def fir_fft_size(n_taps):
    """The transform length fir() picks for n_taps taps: the next power of two >= 4 M, clamped to 256 ... 4096 (the rule of
    smfft_amd.fir_fft_size)."""
    return _bank.fir_fft_size(n_taps)


def fir(x, taps, mode="convolve", fft_size=None):
    """x: (C, L) or (L,) real signal, taps: (K, M) or (M,) real filters (host arrays, cast to float32) -> (C, K, L) float32:
    out[c, k] = np.convolve(x[c], taps[k])[:L] (mode="convolve") or np.correlate(np.r_[x[c], zeros(M-1)], taps[k], 'valid')
    (mode="correlate"), through the overlap-save kernel with N = fft_size (None: fir_fft_size(M)).  Complex input raises TypeError:
    nothing drops an imaginary part (complex data: smfft_amd.fir)."""
    return _bank.fir(x, taps, mode, fft_size)

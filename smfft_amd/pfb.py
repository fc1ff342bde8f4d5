"""ctypes mirror of include/smfft_pfb.h: the critically sampled polyphase filter bank channelizer -- a prototype of P N real taps and an
N-point forward FFT across its P polyphase branches, N = 256 ... 4096, 1 <= P <= 32, fused into one kernel (libsmfft_pfb.so).

The library is loaded on first use, so that `import smfft_amd` behaves the same whether it was built or not.  Device pointers are
plain integers; timings are ADDED to a running total, as in smfft_amd.api.  There is no CPU fallback: a missing library raises on
first call.
"""
from . import _addon, _pfb_bank
from ._pfb_bank import MAX_TAPS_PER_CHANNEL, SIZES  # noqa: F401

# name -> (restype, argtypes), exactly the declarations of include/smfft_pfb.h (tests/test_pfb_cpu.py compares them)
SIGS = _pfb_bank.sigs("smfft_pfb")

LIB_PATH, load, lib = _addon.loader("libsmfft_pfb.so", "SMFFT_PFB_LIB", __name__, SIGS)
_lib = None
_bank = _pfb_bank.Bank("pfb", "smfft_pfb", lib, real=False)


def frames(L, n_channels, taps_per_channel):
    """F = floor(L / N) - P + 1 (0 if not positive): the output frames of one stream of L samples (smfft_pfb_frames)"""
    return _bank.frames(L, n_channels, taps_per_channel)


def default_tile_run(n_channels, taps_per_channel):
    """the schedule's run length of a plain launch (smfft_pfb_default_tile_run)"""
    return _bank.default_tile_run(n_channels, taps_per_channel)


def launch(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, d_output, power=False, stream=0):
    """The channelizer, launch only (no events, no sync): d_output[(c*F + f)*N + k] = sum_m h[m] x_c[f*N + m] exp(-2 pi i k m / N)
    (complex64), or its squared magnitude (float32) with power=True (smfft_pfb_launch)."""
    _bank.launch(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, d_output, power, stream)


def launch_tuned(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, d_output, tile_run, power=False, stream=0):
    """Tuning and tests only: launch with the schedule's run length tile_run (>= 1; 0 = the shipped default).  Same bits for every
    value (smfft_pfb_launch_tuned)."""
    _bank.launch_tuned(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, d_output, tile_run, power, stream)


def benchmark(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, d_output, power=False):
    """One launch on the null stream, timed with events; synchronous.  Returns (status, elapsed_ms)."""
    return _bank.benchmark(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, d_output, power)


def prototype(n_channels, taps_per_channel, window="hamming"):
    """The usual prototype low-pass of P N taps: sinc((m - (P N - 1) / 2) / N) w[m], w = the named window of numpy ("hamming", "hanning",
    "blackman", "bartlett") or "rectangular"; computed in fp64, returned as float32 (rounded once)."""
    return _bank.prototype(n_channels, taps_per_channel, window)


def channelize(x, taps, n_channels, power=False):
    """x: (C, L) or (L,) complex signal, taps: P N real coefficients (host arrays) -> (C, F, N) complex64 spectra, or float32 powers
    with power=True; F = floor(L / N) - P + 1."""
    return _bank.channelize(x, taps, n_channels, power)

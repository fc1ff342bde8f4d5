"""ctypes mirror of include/smfft_pfb_real.h: the critically sampled polyphase filter bank channelizer for real streams -- a prototype of
P 2N real taps and a 2N-point real-to-complex transform across its P polyphase branches, N = 256 ... 4096 channels, 1 <= P <= 32, fused
into one kernel (libsmfft_pfb_real.so).  The complex bank is smfft_amd.pfb.

The library is loaded on first use, so that `import smfft_amd` behaves the same whether it was built or not.  Device pointers are
plain integers; timings are ADDED to a running total, as in smfft_amd.api.  There is no CPU fallback: a missing library raises on
first call.
"""
import numpy as np

from . import _addon, _pfb_bank
from ._pfb_bank import MAX_TAPS_PER_CHANNEL, SIZES  # noqa: F401

# name -> (restype, argtypes), exactly the declarations of include/smfft_pfb_real.h (tests/test_pfb_real_cpu.py compares them)
SIGS = _pfb_bank.sigs("smfft_pfb_real")

LIB_PATH, load, lib = _addon.loader("libsmfft_pfb_real.so", "SMFFT_PFB_REAL_LIB", __name__, SIGS)
_lib = None
_bank = _pfb_bank.Bank("pfb_real", "smfft_pfb_real", lib, real=True)


def frames(L, n_channels, taps_per_channel):
    """F = floor(L / 2N) - P + 1 (0 if not positive): the output frames of one stream of L real samples, L even (smfft_pfb_real_frames)"""
    return _bank.frames(L, n_channels, taps_per_channel)


def default_tile_run(n_channels, taps_per_channel):
    """the schedule's run length of a plain launch (smfft_pfb_real_default_tile_run)"""
    return _bank.default_tile_run(n_channels, taps_per_channel)


def launch(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, d_output, power=False, stream=0):
    """The channelizer, launch only (no events, no sync): d_output[(c*F + f)*N + k] = X_f[k] = sum_m h[m] x_c[2fN + m] exp(-2 pi i k m / 2N)
    for 1 <= k < N and (X_f[0], X_f[N]) at k = 0 (complex64), or |X_f[k]|^2 with X_f[0]^2 at k = 0 (float32) with power=True
    (smfft_pfb_real_launch)."""
    _bank.launch(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, d_output, power, stream)


def launch_tuned(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, d_output, tile_run, power=False, stream=0):
    """Tuning and tests only: launch with the schedule's run length tile_run (>= 1; 0 = the shipped default).  Same bits for every
    value (smfft_pfb_real_launch_tuned)."""
    _bank.launch_tuned(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, d_output, tile_run, power, stream)


def benchmark(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, d_output, power=False):
    """One launch on the null stream, timed with events; synchronous.  Returns (status, elapsed_ms)."""
    return _bank.benchmark(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, d_output, power)


def prototype(n_channels, taps_per_channel, window="hamming"):
    """The usual prototype low-pass of P 2N taps: sinc((m - (2 P N - 1) / 2) / 2N) w[m], w = the named window of numpy ("hamming",
    "hanning", "blackman", "bartlett") or "rectangular"; computed in fp64, returned as float32 (rounded once)."""
    return _bank.prototype(n_channels, taps_per_channel, window)


def unpack(packed):
    """(..., N) complex rows as the device writes them -- element 0 = (X[0], X[N]) -- -> (..., N + 1) rows in np.fft.rfft layout"""
    packed = np.asarray(packed)
    out = np.empty(packed.shape[:-1] + (packed.shape[-1] + 1,), packed.dtype)
    out[..., :-1] = packed
    out[..., 0] = packed[..., 0].real
    out[..., -1] = packed[..., 0].imag
    return out


def channelize(x, taps, n_channels, power=False, packed=False):
    """x: (C, L) or (L,) real signal, taps: P 2N real coefficients (host arrays) -> complex64 spectra (C, F, N + 1) in np.fft.rfft layout
    (unpacked on the host), or (C, F, N) as the device wrote them with packed=True (element 0 = (X[0], X[N])), or float32 powers
    (C, F, N) with power=True (element 0 = X[0]^2; no Nyquist power); F = floor(L / 2N) - P + 1.  L must be even."""
    out = _bank.channelize(x, taps, n_channels, power)
    return out if power or packed else unpack(out)

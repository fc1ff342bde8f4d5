"""ctypes mirror of include/smfft_large_pfb.h: the critically sampled polyphase filter bank channelizer of smfft_amd.pfb for N = 8192 and
16384 channels -- a prototype of P N real taps and an N-point forward FFT across its P polyphase branches, 1 <= P <= 32, fused into one
kernel on the single-pass engine of smfft_amd.large (libsmfft_large_pfb.so).

The library is loaded on first use, so that `import smfft_amd` behaves the same whether it was built or not.  Device pointers are
plain integers; timings are ADDED to a running total, as in smfft_amd.api.  There is no CPU fallback: a missing library raises on
first call.
"""
import ctypes

from . import _addon, _pfb_bank
from ._pfb_bank import MAX_TAPS_PER_CHANNEL  # noqa: F401

SIZES = (8192, 16384)
STRIDE, XCD_BLOCKED = 1, 2      # the schedules of launch_tuned

_PREFIX = "smfft_large_pfb"
_i = ctypes.c_int
# name -> (restype, argtypes), exactly the declarations of include/smfft_large_pfb.h (tests/test_large_pfb_cpu.py compares them): the
# complex bank's frames / launch / benchmark, a tuned launch that takes the schedule and the grid, and the default schedule
SIGS = {name: sig for name, sig in _pfb_bank.sigs(_PREFIX).items() if name.split(_PREFIX)[1] in ("_frames", "_launch", "_benchmark")}
SIGS[_PREFIX + "_launch_tuned"] = (_i, SIGS[_PREFIX + "_launch"][1] + [_i, _i])
SIGS[_PREFIX + "_default_schedule"] = (_i, [_i, _i])

LIB_PATH, load, lib = _addon.loader("libsmfft_large_pfb.so", "SMFFT_LARGE_PFB_LIB", __name__, SIGS)
_lib = None
_bank = _pfb_bank.Bank("large_pfb", _PREFIX, lib, real=False, sizes=SIZES)


def frames(L, n_channels, taps_per_channel):
    """F = floor(L / N) - P + 1 (0 if not positive): the output frames of one stream of L samples (smfft_large_pfb_frames)"""
    return _bank.frames(L, n_channels, taps_per_channel)


def default_schedule(n_channels, taps_per_channel):
    """the schedule of a plain launch: STRIDE or XCD_BLOCKED (smfft_large_pfb_default_schedule)"""
    s = _bank.call("default_schedule", n_channels, taps_per_channel)
    if s < 0:
        raise ValueError(f"{_PREFIX}_default_schedule(N={n_channels}, P={taps_per_channel}) -> {s}")
    return s


def launch(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, d_output, power=False, stream=0):
    """The channelizer, launch only (no events, no sync): d_output[(c*F + f)*N + k] = sum_m h[m] x_c[f*N + m] exp(-2 pi i k m / N)
    (complex64), or its squared magnitude (float32) with power=True (smfft_large_pfb_launch)."""
    _bank.launch(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, d_output, power, stream)


def launch_tuned(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, d_output, schedule=0, max_workgroups=0, power=False, stream=0):
    """Tuning and tests only: launch with the schedule (STRIDE, XCD_BLOCKED; 0 = the shipped default) and at most max_workgroups
    workgroups (0 = what the device holds at once).  Same bits for every value (smfft_large_pfb_launch_tuned)."""
    rc = _bank.call("launch_tuned", d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, int(bool(power)), d_output, stream, schedule, max_workgroups)
    if rc != 0:
        raise RuntimeError(f"{_PREFIX}_launch_tuned(L={L}, C={n_streams}, N={n_channels}, P={taps_per_channel}, schedule={schedule}, "
                           f"max_workgroups={max_workgroups}) -> {rc}")


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

"""ctypes mirror of include/smfft_pfb_spec.h: integrated power spectra of the polyphase filter banks -- the power of every channel summed
over n_integrate consecutive frames inside the channelizer's kernel, for complex streams (the bank of smfft_amd.pfb) and, with real=True,
for real streams (the bank of smfft_amd.pfb_real); N = 256 ... 4096 channels, 1 <= P <= 32 (libsmfft_pfb_spec.so).

The library is loaded on first use, so that `import smfft_amd` behaves the same whether it was built or not.  Device pointers are
plain integers; timings are ADDED to a running total, as in smfft_amd.api.  There is no CPU fallback: a missing library raises on
first call.
"""
import ctypes

import numpy as np

from . import _addon, _pfb_bank
from ._pfb_bank import MAX_TAPS_PER_CHANNEL, SIZES  # noqa: F401

_vp, _i, _ll, _dp = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.POINTER(ctypes.c_double)
PREFIXES = ("smfft_pfb_spec", "smfft_pfb_real_spec")       # complex streams, real streams


def _sigs(prefix):
    return {
        prefix + "_spectra": (_ll, [_ll, _i, _i, _i]),
        prefix + "_launch": (_i, [_vp, _ll, _i, _vp, _i, _i, _i, _vp, _vp]),
        prefix + "_benchmark": (_i, [_vp, _ll, _i, _vp, _i, _i, _i, _vp, _dp]),
        prefix + "_launch_tuned": (_i, [_vp, _ll, _i, _vp, _i, _i, _i, _vp, _vp, _i]),
    }


# name -> (restype, argtypes), exactly the declarations of include/smfft_pfb_spec.h (tests/test_pfb_spec_cpu.py compares them)
SIGS = {**_sigs(PREFIXES[0]), **_sigs(PREFIXES[1])}

LIB_PATH, load, lib = _addon.loader("libsmfft_pfb_spec.so", "SMFFT_PFB_SPEC_LIB", __name__, SIGS)
_lib = None
_banks = tuple(_pfb_bank.Bank("pfb_spec", prefix, lib, real=real) for real, prefix in enumerate(PREFIXES))      # complex streams, real streams


def _fn(name, real):
    return getattr(lib(), f"{PREFIXES[bool(real)]}_{name}")


def spectra(L, n_channels, taps_per_channel, n_integrate, real=False):
    """I = floor(F / n_integrate), F the frames of one stream of L samples as the bank counts them (smfft_pfb_spec_spectra /
    smfft_pfb_real_spec_spectra)"""
    n = _fn("spectra", real)(L, n_channels, taps_per_channel, n_integrate)
    if n < 0:
        raise ValueError(f"{PREFIXES[bool(real)]}_spectra(L={L}, N={n_channels}, P={taps_per_channel}, T={n_integrate}) -> {n}: N must be one of "
                         f"{SIZES}, 1 <= P <= {MAX_TAPS_PER_CHANNEL}, T >= 1, L >= 0" + (" and even" if real else ""))
    return n


def launch(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, n_integrate, d_output, real=False, stream=None):
    """Launch only (no events, no sync): d_output[(c*I + i)*N + k] = sum_{t < n_integrate} p[c, i*n_integrate + t, k] in float32, p what
    the bank's power mode stores for that frame, summed in frame order (smfft_pfb_spec_launch / smfft_pfb_real_spec_launch)."""
    rc = _fn("launch", real)(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, n_integrate, d_output, stream)
    if rc != 0:
        raise RuntimeError(f"{PREFIXES[bool(real)]}_launch(L={L}, C={n_streams}, N={n_channels}, P={taps_per_channel}, T={n_integrate}) -> {rc}")


def launch_tuned(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, n_integrate, d_output, max_workgroups, real=False, stream=None):
    """Tuning and tests only: launch on at most max_workgroups workgroups (>= 1; 0 = the shipped grid).  Same bits for every value
    (smfft_pfb_spec_launch_tuned / smfft_pfb_real_spec_launch_tuned)."""
    rc = _fn("launch_tuned", real)(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, n_integrate, d_output, stream, max_workgroups)
    if rc != 0:
        raise RuntimeError(f"{PREFIXES[bool(real)]}_launch_tuned(L={L}, C={n_streams}, N={n_channels}, P={taps_per_channel}, T={n_integrate}, "
                           f"G={max_workgroups}) -> {rc}")


def benchmark(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, n_integrate, d_output, real=False):
    """One launch on the null stream, timed with events; synchronous.  Returns (status, elapsed_ms)."""
    t = ctypes.c_double(0.0)
    rc = _fn("benchmark", real)(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, n_integrate, d_output, ctypes.byref(t))
    return rc, t.value


def prototype(n_channels, taps_per_channel, window="hamming", real=False):
    """the prototype low-pass of the bank: smfft_amd.pfb.prototype (P N taps), or smfft_amd.pfb_real.prototype (P 2N taps) with real=True"""
    return _banks[bool(real)].prototype(n_channels, taps_per_channel, window)


def integrate(x, taps, n_channels, n_integrate, real=False):
    """x: (C, L) or (L,) signal (complex, or real with real=True), taps: P N (real=True: P 2N) real coefficients (host arrays) ->
    float32 integrated power spectra (C, I, N), I = spectra(L, N, P, n_integrate, real)."""
    T = int(n_integrate)
    return _banks[bool(real)].round_trip(
        x, taps, n_channels, lambda L, N, P: spectra(L, N, P, T, real), np.float32,
        lambda d_signal, L, C, d_taps, N, P, d_output: _fn("launch", real)(d_signal, L, C, d_taps, N, P, T, d_output, None),
        "x must be (C, L) or (L,), taps a vector", "the prototype must be real" + (", and so must the signal with real=True" if real else ""),
        "integrate", f", T={T}, real={bool(real)}")

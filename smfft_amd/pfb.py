"""ctypes mirror of include/smfft_pfb.h: the critically sampled polyphase filter bank channelizer -- a prototype of P N real taps and an
N-point forward FFT across its P polyphase branches, N = 256 ... 4096, 1 <= P <= 32, fused into one kernel (libsmfft_pfb.so).

The library is loaded on first use, so that `import smfft_amd` behaves the same whether it was built or not.  Device pointers are
plain integers; timings are ADDED to a running total, as in smfft_amd.api.  There is no CPU fallback: a missing library raises on
first call.
"""
import ctypes

import numpy as np

from . import _addon

SIZES = (256, 512, 1024, 2048, 4096)
MAX_TAPS_PER_CHANNEL = 32

_vp, _i, _ll, _dp = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.POINTER(ctypes.c_double)
# name -> (restype, argtypes), exactly the declarations of include/smfft_pfb.h (tests/test_pfb_cpu.py compares them)
SIGS = {
    "smfft_pfb_frames": (_ll, [_ll, _i, _i]),
    "smfft_pfb_launch": (_i, [_vp, _ll, _i, _vp, _i, _i, _i, _vp, _vp]),
    "smfft_pfb_benchmark": (_i, [_vp, _ll, _i, _vp, _i, _i, _i, _vp, _dp]),
    "smfft_pfb_launch_tuned": (_i, [_vp, _ll, _i, _vp, _i, _i, _i, _vp, _vp, _i]),
    "smfft_pfb_default_tile_run": (_i, [_i, _i]),
}

LIB_PATH, load, lib = _addon.loader("libsmfft_pfb.so", "SMFFT_PFB_LIB", __name__, SIGS)
_lib = None


def frames(L, n_channels, taps_per_channel):
    """F = floor(L / N) - P + 1 (0 if not positive): the output frames of one stream of L samples (smfft_pfb_frames)"""
    f = lib().smfft_pfb_frames(L, n_channels, taps_per_channel)
    if f < 0:
        raise ValueError(f"smfft_pfb_frames(L={L}, N={n_channels}, P={taps_per_channel}) -> {f}: N must be one of {SIZES}, "
                         f"1 <= P <= {MAX_TAPS_PER_CHANNEL}, L >= 0")
    return f


def default_tile_run(n_channels, taps_per_channel):
    """the schedule's run length of a plain launch (smfft_pfb_default_tile_run)"""
    r = lib().smfft_pfb_default_tile_run(n_channels, taps_per_channel)
    if r < 0:
        raise ValueError(f"smfft_pfb_default_tile_run(N={n_channels}, P={taps_per_channel}) -> {r}")
    return r


def launch(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, d_output, power=False, stream=0):
    """The channelizer, launch only (no events, no sync): d_output[(c*F + f)*N + k] = sum_m h[m] x_c[f*N + m] exp(-2 pi i k m / N)
    (complex64), or its squared magnitude (float32) with power=True (smfft_pfb_launch)."""
    rc = lib().smfft_pfb_launch(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, int(bool(power)), d_output, stream)
    if rc != 0:
        raise RuntimeError(f"smfft_pfb_launch(L={L}, C={n_streams}, N={n_channels}, P={taps_per_channel}) -> {rc}")


def launch_tuned(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, d_output, tile_run, power=False, stream=0):
    """Tuning and tests only: launch with the schedule's run length tile_run (>= 1; 0 = the shipped default).  Same bits for every
    value (smfft_pfb_launch_tuned)."""
    rc = lib().smfft_pfb_launch_tuned(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, int(bool(power)), d_output, stream, tile_run)
    if rc != 0:
        raise RuntimeError(f"smfft_pfb_launch_tuned(L={L}, C={n_streams}, N={n_channels}, P={taps_per_channel}, R={tile_run}) -> {rc}")


def benchmark(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, d_output, power=False):
    """One launch on the null stream, timed with events; synchronous.  Returns (status, elapsed_ms)."""
    t = ctypes.c_double(0.0)
    rc = lib().smfft_pfb_benchmark(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, int(bool(power)), d_output, ctypes.byref(t))
    return rc, t.value


def prototype(n_channels, taps_per_channel, window="hamming"):
    """The usual prototype low-pass of P N taps: sinc((m - (P N - 1) / 2) / N) w[m], w = the named window of numpy ("hamming", "hanning",
    "blackman", "bartlett") or "rectangular"; computed in fp64, returned as float32 (rounded once)."""
    N, P = int(n_channels), int(taps_per_channel)
    if N < 1 or P < 1:
        raise ValueError(f"prototype(N={N}, P={P})")
    M = P * N
    if window == "rectangular":
        w = np.ones(M)
    elif window in ("hamming", "hanning", "blackman", "bartlett"):
        w = getattr(np, window)(M)
    else:
        raise ValueError(f"unknown window {window!r}")
    m = np.arange(M, dtype=np.float64)
    return (np.sinc((m - (M - 1) / 2) / N) * w).astype(np.float32)


def channelize(x, taps, n_channels, power=False):
    """x: (C, L) or (L,) complex signal, taps: P N real coefficients (host arrays) -> (C, F, N) complex64 spectra, or float32 powers
    with power=True; F = floor(L / N) - P + 1."""
    x, taps = np.asarray(x), np.asarray(taps)
    if x.ndim not in (1, 2) or taps.ndim != 1:
        raise ValueError("x must be (C, L) or (L,), taps a vector of P N coefficients")
    if np.iscomplexobj(taps):
        raise ValueError("the prototype must be real")
    N = int(n_channels)
    if N not in SIZES or taps.size % N or not 1 <= taps.size // N <= MAX_TAPS_PER_CHANNEL:
        raise ValueError(f"smfft_amd.pfb serves N in {SIZES} with P N taps, 1 <= P <= {MAX_TAPS_PER_CHANNEL}, not N = {N} with {taps.size} taps")
    P = taps.size // N
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.complex64)
    taps = np.ascontiguousarray(taps, dtype=np.float32)
    C, L = x.shape
    F = frames(L, N, P)
    dtype, width = (np.float32, 4) if power else (np.complex64, 8)
    if C * F == 0:
        return np.empty((C, F, N), dtype)
    from . import api      # the device allocator and copies of libsmfft_amd.so
    din, dtaps = api.DeviceBuffer.from_host(x), api.DeviceBuffer.from_host(taps)
    dout = api.DeviceBuffer(C * F * N * width)
    api.lib.smfft_memset(dout.ptr, 0xFF, dout.nbytes)   # NaN pattern: untouched outputs are caught
    rc = lib().smfft_pfb_launch(din.ptr, L, C, dtaps.ptr, N, P, int(bool(power)), dout.ptr, None)
    if rc == 0:
        rc = api.lib.smfft_synchronize()
    if rc != 0:
        raise RuntimeError(f"pfb.channelize(C={C}, L={L}, N={N}, P={P}) -> {rc}")
    out = dout.to_host(dtype, (C, F, N))
    for b in (din, dtaps, dout):
        b.free()
    return out

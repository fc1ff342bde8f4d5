"""ctypes mirror of include/smfft_pfb_real.h: the critically sampled polyphase filter bank channelizer for real streams -- a prototype of
P 2N real taps and a 2N-point real-to-complex transform across its P polyphase branches, N = 256 ... 4096 channels, 1 <= P <= 32, fused
into one kernel (libsmfft_pfb_real.so).  The complex bank is smfft_amd.pfb.

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
# name -> (restype, argtypes), exactly the declarations of include/smfft_pfb_real.h (tests/test_pfb_real_cpu.py compares them)
SIGS = {
    "smfft_pfb_real_frames": (_ll, [_ll, _i, _i]),
    "smfft_pfb_real_launch": (_i, [_vp, _ll, _i, _vp, _i, _i, _i, _vp, _vp]),
    "smfft_pfb_real_benchmark": (_i, [_vp, _ll, _i, _vp, _i, _i, _i, _vp, _dp]),
    "smfft_pfb_real_launch_tuned": (_i, [_vp, _ll, _i, _vp, _i, _i, _i, _vp, _vp, _i]),
    "smfft_pfb_real_default_tile_run": (_i, [_i, _i]),
}

LIB_PATH, load, lib = _addon.loader("libsmfft_pfb_real.so", "SMFFT_PFB_REAL_LIB", __name__, SIGS)
_lib = None


def frames(L, n_channels, taps_per_channel):
    """F = floor(L / 2N) - P + 1 (0 if not positive): the output frames of one stream of L real samples, L even (smfft_pfb_real_frames)"""
    f = lib().smfft_pfb_real_frames(L, n_channels, taps_per_channel)
    if f < 0:
        raise ValueError(f"smfft_pfb_real_frames(L={L}, N={n_channels}, P={taps_per_channel}) -> {f}: N must be one of {SIZES}, "
                         f"1 <= P <= {MAX_TAPS_PER_CHANNEL}, L >= 0 and even")
    return f


def default_tile_run(n_channels, taps_per_channel):
    """the schedule's run length of a plain launch (smfft_pfb_real_default_tile_run)"""
    r = lib().smfft_pfb_real_default_tile_run(n_channels, taps_per_channel)
    if r < 0:
        raise ValueError(f"smfft_pfb_real_default_tile_run(N={n_channels}, P={taps_per_channel}) -> {r}")
    return r


def launch(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, d_output, power=False, stream=0):
    """The channelizer, launch only (no events, no sync): d_output[(c*F + f)*N + k] = X_f[k] = sum_m h[m] x_c[2fN + m] exp(-2 pi i k m / 2N)
    for 1 <= k < N and (X_f[0], X_f[N]) at k = 0 (complex64), or |X_f[k]|^2 with X_f[0]^2 at k = 0 (float32) with power=True
    (smfft_pfb_real_launch)."""
    rc = lib().smfft_pfb_real_launch(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, int(bool(power)), d_output, stream)
    if rc != 0:
        raise RuntimeError(f"smfft_pfb_real_launch(L={L}, C={n_streams}, N={n_channels}, P={taps_per_channel}) -> {rc}")


def launch_tuned(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, d_output, tile_run, power=False, stream=0):
    """Tuning and tests only: launch with the schedule's run length tile_run (>= 1; 0 = the shipped default).  Same bits for every
    value (smfft_pfb_real_launch_tuned)."""
    rc = lib().smfft_pfb_real_launch_tuned(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, int(bool(power)), d_output, stream, tile_run)
    if rc != 0:
        raise RuntimeError(f"smfft_pfb_real_launch_tuned(L={L}, C={n_streams}, N={n_channels}, P={taps_per_channel}, R={tile_run}) -> {rc}")


def benchmark(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, d_output, power=False):
    """One launch on the null stream, timed with events; synchronous.  Returns (status, elapsed_ms)."""
    t = ctypes.c_double(0.0)
    rc = lib().smfft_pfb_real_benchmark(d_signal, L, n_streams, d_taps, n_channels, taps_per_channel, int(bool(power)), d_output, ctypes.byref(t))
    return rc, t.value


def prototype(n_channels, taps_per_channel, window="hamming"):
    """The usual prototype low-pass of P 2N taps: sinc((m - (2 P N - 1) / 2) / 2N) w[m], w = the named window of numpy ("hamming",
    "hanning", "blackman", "bartlett") or "rectangular"; computed in fp64, returned as float32 (rounded once)."""
    N, P = int(n_channels), int(taps_per_channel)
    if N < 1 or P < 1:
        raise ValueError(f"prototype(N={N}, P={P})")
    M = 2 * P * N
    if window == "rectangular":
        w = np.ones(M)
    elif window in ("hamming", "hanning", "blackman", "bartlett"):
        w = getattr(np, window)(M)
    else:
        raise ValueError(f"unknown window {window!r}")
    m = np.arange(M, dtype=np.float64)
    return (np.sinc((m - (M - 1) / 2) / (2 * N)) * w).astype(np.float32)


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
    x, taps = np.asarray(x), np.asarray(taps)
    if x.ndim not in (1, 2) or taps.ndim != 1:
        raise ValueError("x must be (C, L) or (L,), taps a vector of P 2N coefficients")
    if np.iscomplexobj(x) or np.iscomplexobj(taps):
        raise ValueError("the signal and the prototype must be real (complex signals: smfft_amd.pfb)")
    N = int(n_channels)
    if N not in SIZES or taps.size % (2 * N) or not 1 <= taps.size // (2 * N) <= MAX_TAPS_PER_CHANNEL:
        raise ValueError(f"smfft_amd.pfb_real serves N in {SIZES} with P 2N taps, 1 <= P <= {MAX_TAPS_PER_CHANNEL}, not N = {N} with {taps.size} taps")
    P = taps.size // (2 * N)
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float32)
    taps = np.ascontiguousarray(taps, dtype=np.float32)
    C, L = x.shape
    F = frames(L, N, P)
    dtype, width = (np.float32, 4) if power else (np.complex64, 8)
    if C * F == 0:
        return np.empty((C, F, N if power or packed else N + 1), dtype)
    from . import api      # the device allocator and copies of libsmfft_amd.so
    din, dtaps = api.DeviceBuffer.from_host(x), api.DeviceBuffer.from_host(taps)
    dout = api.DeviceBuffer(C * F * N * width)
    api.lib.smfft_memset(dout.ptr, 0xFF, dout.nbytes)   # NaN pattern: untouched outputs are caught
    rc = lib().smfft_pfb_real_launch(din.ptr, L, C, dtaps.ptr, N, P, int(bool(power)), dout.ptr, None)
    if rc == 0:
        rc = api.lib.smfft_synchronize()
    if rc != 0:
        raise RuntimeError(f"pfb_real.channelize(C={C}, L={L}, N={N}, P={P}) -> {rc}")
    out = dout.to_host(dtype, (C, F, N))
    for b in (din, dtaps, dout):
        b.free()
    return out if power or packed else unpack(out)

"""ctypes mirror of include/smfft_mdct.h: batched DCT-IV / DST-IV of real rows of n = 512 ... 8192 points (powers of two) and the MDCT /
IMDCT of N = 512 ... 8192 coefficients per frame of 2 N samples, each in one kernel (libsmfft_mdct.so: the even and the reversed odd
samples in the two lanes of one complex transform of M = n / 2 points on the register engine, one twiddle in front of it and one behind
it).  float32 in, float32 out, un-normalised:

    dct4(x)[k] = 2 sum_j x[j] cos(pi (2k+1)(2j+1) / (4n))                     = scipy.fft.dct(x, 4);  dct4(dct4(x)) = 2n x
    dst4(x)[k] = 2 sum_j x[j] sin(pi (2k+1)(2j+1) / (4n))                     = scipy.fft.dst(x, 4)
    mdct(x, w)[k] = sum_{j<2N} w[j] x[j] cos(pi/N (j + 1/2 + N/2)(k + 1/2)),   k < N
    imdct(X, w)[j] = w[j] sum_{k<N} X[k] cos(pi/N (j + 1/2 + N/2)(k + 1/2)),   j < 2N

With w[j]^2 + w[j+N]^2 = 1 (sine_window), overlap_add(imdct(mdct_frames(s, w, N), w)) = (N/2) s away from the first and the last N
samples.

The library is loaded on first use, so that `import smfft_amd` behaves the same whether it was built or not.  dct4 / dst4 / mdct /
mdct_frames / imdct take tensors on the device (dct4 / dst4 host arrays as well); the *_ptr, *_tuned and *_benchmark forms take device
pointers as plain integers.  There is no plan and nothing to prepare; timings are ADDED to a running total, as in smfft_amd.api.
Refusals are raised before a device is touched.  There is no CPU fallback: a missing library raises on first call.
"""
import ctypes

import numpy as np

from . import _addon
from ._rows import check_tensor as _check_tensor
from ._rows import host_round_trip as _host_round_trip

SIZES = (256, 512, 1024, 2048, 4096)          # the inner transform lengths M = n / 2
LENGTHS = (512, 1024, 2048, 4096, 8192)       # the row lengths n, and the coefficients per frame N

_vp, _i, _ll, _dp = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.POINTER(ctypes.c_double)
_DCT4 = [_vp, _vp, _i, _ll, _i]               # d_in, d_out, n, batch, sine
_MDCT = [_vp, _vp, _vp, _i, _ll, _ll, _ll, _ll]   # d_in, d_out, d_window, N, streams, frames, hop, stream_stride
_IMDCT = [_vp, _vp, _vp, _i, _ll]             # d_in, d_out, d_window, N, batch
# name -> (restype, argtypes), exactly the declarations of include/smfft_mdct.h (tests/test_sm_mdct_cpu.py compares them)
SIGS = {
    "smfft_mdct_fft_size": (_i, [_i]),
    "smfft_dct4_launch": (_i, _DCT4 + [_vp]),
    "smfft_dct4_launch_tuned": (_i, _DCT4 + [_vp, _i]),
    "smfft_dct4_benchmark": (_i, _DCT4 + [_dp]),
    "smfft_mdct_launch": (_i, _MDCT + [_vp]),
    "smfft_mdct_launch_tuned": (_i, _MDCT + [_vp, _i]),
    "smfft_mdct_benchmark": (_i, _MDCT + [_dp]),
    "smfft_imdct_launch": (_i, _IMDCT + [_vp]),
    "smfft_imdct_launch_tuned": (_i, _IMDCT + [_vp, _i]),
    "smfft_imdct_benchmark": (_i, _IMDCT + [_dp]),
}

LIB_PATH, load, lib = _addon.loader("libsmfft_mdct.so", "SMFFT_MDCT_LIB", __name__, SIGS)
_lib = None


def _check(n):
    n = int(n)
    if n not in LENGTHS:
        raise ValueError(f"smfft_amd.mdct serves n (N) in {LENGTHS}, not {n}")
    return n


def _raise(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} -> {rc}")


def fft_size(n):
    """M = n / 2, the length of the kernels' complex transform (smfft_mdct_fft_size)"""
    return lib().smfft_mdct_fft_size(_check(n))


# ---- device pointers -------------------------------------------------------------------------------------------------------------------
def dct4_ptr(d_in, d_out, n, batch, sine=False, stream=0, grid=None):
    """batch DCT-IV (DST-IV: sine) transforms of float32 rows of n points from d_in to d_out (device pointers; d_out == d_in is
    allowed), launch only (smfft_dct4_launch; grid: on that many workgroups, smfft_dct4_launch_tuned)"""
    if grid is None:
        rc = lib().smfft_dct4_launch(d_in, d_out, n, batch, int(bool(sine)), stream)
    else:
        rc = lib().smfft_dct4_launch_tuned(d_in, d_out, n, batch, int(bool(sine)), stream, grid)
    _raise(rc, f"smfft_dct4_launch(n={n}, batch={batch}, sine={bool(sine)}, grid={grid})")


def mdct_ptr(d_in, d_out, d_window, N, streams, frames, hop, stream_stride, stream=0, grid=None):
    """streams * frames MDCTs: frame (c, f) reads d_in[c stream_stride + f hop ... + 2N) and writes d_out[(c frames + f) N ... + N);
    d_window: 2N floats or None (smfft_mdct_launch; grid: smfft_mdct_launch_tuned)"""
    if grid is None:
        rc = lib().smfft_mdct_launch(d_in, d_out, d_window, N, streams, frames, hop, stream_stride, stream)
    else:
        rc = lib().smfft_mdct_launch_tuned(d_in, d_out, d_window, N, streams, frames, hop, stream_stride, stream, grid)
    _raise(rc, f"smfft_mdct_launch(N={N}, streams={streams}, frames={frames}, hop={hop}, stream_stride={stream_stride}, grid={grid})")


def imdct_ptr(d_in, d_out, d_window, N, batch, stream=0, grid=None):
    """batch IMDCTs: rows of N coefficients at d_in, rows of 2N samples at d_out (smfft_imdct_launch; grid: smfft_imdct_launch_tuned)"""
    if grid is None:
        rc = lib().smfft_imdct_launch(d_in, d_out, d_window, N, batch, stream)
    else:
        rc = lib().smfft_imdct_launch_tuned(d_in, d_out, d_window, N, batch, stream, grid)
    _raise(rc, f"smfft_imdct_launch(N={N}, batch={batch}, grid={grid})")


launch_ptr = dct4_ptr


def dct4_benchmark(d_in, d_out, n, batch, sine=False):
    """One launch on the null stream, timed with events; synchronous.  Returns (status, elapsed_ms)."""
    t = ctypes.c_double(0.0)
    rc = lib().smfft_dct4_benchmark(d_in, d_out, n, batch, int(bool(sine)), ctypes.byref(t))
    return rc, t.value


def mdct_benchmark(d_in, d_out, d_window, N, streams, frames, hop, stream_stride):
    t = ctypes.c_double(0.0)
    rc = lib().smfft_mdct_benchmark(d_in, d_out, d_window, N, streams, frames, hop, stream_stride, ctypes.byref(t))
    return rc, t.value


def imdct_benchmark(d_in, d_out, d_window, N, batch):
    t = ctypes.c_double(0.0)
    rc = lib().smfft_imdct_benchmark(d_in, d_out, d_window, N, batch, ctypes.byref(t))
    return rc, t.value


# ---- tensors ---------------------------------------------------------------------------------------------------------------------------
def _check_window(window, N, x):
    if window is None:
        return None
    w = _check_tensor(window, "window")
    if w.shape != (2 * N,):
        raise ValueError(f"window must hold 2N = {2 * N} floats, not {tuple(w.shape)}")
    if w.device != x.device:
        raise ValueError(f"window must be on x's device: {w.device} against {x.device}")
    return w


def _on_device(x, what):
    if not x.is_cuda:
        raise ValueError(f"smfft_amd.mdct.{what} takes tensors on the device.  There is no CPU fallback")


def _stream(x, stream):
    import torch
    return torch.cuda.current_stream(x.device).cuda_stream if stream is None else stream


def launch(x, out=None, sine=False, stream=None):
    """DCT-IV / DST-IV.  x: a contiguous float32 torch tensor on the device, rows on the last axis; out: such a tensor of the same
    shape, x itself (in place), or None for a new one.  Enqueues one launch on `stream` (a hipStream_t as an integer; None = torch's
    current stream of x's device) and returns out; nothing is synchronised"""
    x = _check_tensor(x, "x")
    n = _check(x.shape[-1])                                               # (refuses before anything touches a device)
    if out is not None and (_check_tensor(out, "out").shape != x.shape or out.device != x.device):
        raise ValueError(f"out must have x's shape and device: {tuple(out.shape)} on {out.device} against {tuple(x.shape)} on {x.device}")
    _on_device(x, "launch")
    import torch
    handle = lib()
    if out is None:
        out = torch.empty_like(x)
    batch = x.numel() // n
    with torch.cuda.device(x.device):
        rc = handle.smfft_dct4_launch(x.data_ptr(), out.data_ptr(), n, batch, int(bool(sine)), _stream(x, stream))
    _raise(rc, f"smfft_dct4_launch(n={n}, batch={batch}, sine={bool(sine)})")
    return out


def _transform(x, sine):
    if type(x).__module__.split(".")[0] == "torch":                  # a tensor, without importing torch for host arrays
        import torch
        if x.is_cuda:
            return launch(x, None, sine)
        return torch.from_numpy(_transform(x.numpy(), sine))
    x = np.asarray(x)
    if np.iscomplexobj(x):
        raise TypeError("smfft_amd.mdct takes real rows")
    if x.ndim < 1:
        raise ValueError("x must have at least one axis")
    n = _check(x.shape[-1])                                               # (refuses before anything touches a device)
    shape = x.shape
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, n)
    batch = x.shape[0]
    handle = lib()
    return _host_round_trip(x, np.float32, lambda din, dout: handle.smfft_dct4_launch(din, dout, n, batch, int(bool(sine)), None),
                            f"dct4(n={n}, batch={batch}, sine={bool(sine)})").reshape(shape)


def dct4(x):
    """the DCT-IV along the last axis.  x: a contiguous float32 torch tensor on the device -> a new tensor there, from one launch on
    torch's current stream; or a host array / CPU tensor of any real dtype -> float32 of the same shape through a host round trip
    (upload, one launch, download)"""
    return _transform(x, False)


def dst4(x):
    """the DST-IV along the last axis; x as in dct4()"""
    return _transform(x, True)


def mdct(x, window=None, stream=None):
    """the MDCT of rows of 2N samples on the last axis of a contiguous float32 tensor on the device -> (..., N), one launch.
    window: 2N float32 on the same device, or None for all ones"""
    x = _check_tensor(x, "x")
    if x.shape[-1] % 2:
        raise ValueError(f"rows of 2N samples, not {x.shape[-1]}")
    N = _check(x.shape[-1] // 2)
    w = _check_window(window, N, x)
    _on_device(x, "mdct")
    import torch
    handle = lib()
    out = torch.empty(x.shape[:-1] + (N,), dtype=torch.float32, device=x.device)
    rows = x.numel() // (2 * N)
    with torch.cuda.device(x.device):
        rc = handle.smfft_mdct_launch(x.data_ptr(), out.data_ptr(), None if w is None else w.data_ptr(), N, rows, 1, N, 2 * N, _stream(x, stream))
    _raise(rc, f"smfft_mdct_launch(N={N}, streams={rows}, frames=1)")
    return out


def mdct_frames(signal, window, N, stream=None):
    """the lapped transform: signal (C, L) float32 on the device, L a multiple of N and at least 2N -> (C, L / N - 1, N), frame f of
    stream c from signal[c, f N ... f N + 2N), in one launch that reads every sample from the signal itself"""
    s = _check_tensor(signal, "signal", axes=2)
    N = _check(N)
    if s.ndim != 2 or s.shape[1] % N or s.shape[1] < 2 * N:
        raise ValueError(f"signal must be (C, L) with L a multiple of N = {N} and at least 2N, not {tuple(s.shape)}")
    w = _check_window(window, N, s)
    _on_device(s, "mdct_frames")
    import torch
    handle = lib()
    C, L = s.shape
    F = L // N - 1
    out = torch.empty((C, F, N), dtype=torch.float32, device=s.device)
    with torch.cuda.device(s.device):
        rc = handle.smfft_mdct_launch(s.data_ptr(), out.data_ptr(), None if w is None else w.data_ptr(), N, C, F, N, L, _stream(s, stream))
    _raise(rc, f"smfft_mdct_launch(N={N}, streams={C}, frames={F}, hop={N}, stream_stride={L})")
    return out


def imdct(X, window=None, stream=None):
    """the IMDCT of rows of N coefficients on the last axis of a contiguous float32 tensor on the device -> (..., 2N) windowed
    samples, one launch; overlap_add() sums them"""
    X = _check_tensor(X, "X")
    N = _check(X.shape[-1])
    w = _check_window(window, N, X)
    _on_device(X, "imdct")
    import torch
    handle = lib()
    out = torch.empty(X.shape[:-1] + (2 * N,), dtype=torch.float32, device=X.device)
    rows = X.numel() // N
    with torch.cuda.device(X.device):
        rc = handle.smfft_imdct_launch(X.data_ptr(), out.data_ptr(), None if w is None else w.data_ptr(), N, rows, _stream(X, stream))
    _raise(rc, f"smfft_imdct_launch(N={N}, batch={rows})")
    return out


def overlap_add(y):
    """(..., F, 2N) -> (..., (F + 1) N): frame f added at offset f N.  Plain torch operations (two slice additions), not a kernel of
    this library: the IMDCT kernel writes every frame once and adds nothing"""
    import torch
    F, N = y.shape[-2], y.shape[-1] // 2
    out = torch.zeros(y.shape[:-2] + (F + 1, N), dtype=y.dtype, device=y.device)
    out[..., :F, :] += y[..., :N]
    out[..., 1:, :] += y[..., N:]
    return out.reshape(y.shape[:-2] + ((F + 1) * N,))


def sine_window(N, device=None):
    """sin(pi (j + 1/2) / (2N)), j < 2N, computed in fp64 and rounded once: w[j]^2 + w[j+N]^2 = 1"""
    import torch
    N = _check(N)
    w = np.sin(np.pi * (np.arange(2 * N, dtype=np.float64) + 0.5) / (2 * N)).astype(np.float32)
    return torch.from_numpy(w).to(device) if device is not None else torch.from_numpy(w)

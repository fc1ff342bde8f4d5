"""ctypes mirror of include/smfft_hilbert.h: batched Hilbert transform, analytic signal and envelope of real rows of n = 512 ... 8192
points (powers of two) in one kernel (libsmfft_hilbert.so: consecutive pairs of samples in the two lanes of a forward transform of
M = n / 2 points on the register engine, the Hermitian split, the multiplier -i sgn and the C2R merge in one line, an inverse
transform).  float32 in; with X = DFT_n(x) and s[k] = +1 (0 < k < n/2), -1 (n/2 < k < n), 0 (k = 0, n/2):

    hilbert(x)  = IDFT_n(-i s[k] X[k])                 = scipy.signal.hilbert(x).imag        float32, kind 0 (QUADRATURE)
    analytic(x) = x + i hilbert(x)                     ~ scipy.signal.hilbert(x)             complex64, kind 1 (ANALYTIC); .real is x to the bit
    envelope(x) = sqrt(x^2 + hilbert(x)^2)             = abs(scipy.signal.hilbert(x))        float32, kind 2 (ENVELOPE)

The library is loaded on first use, so that `import smfft_amd` behaves the same whether it was built or not.  launch / hilbert /
analytic / envelope take tensors or arrays; launch_ptr, launch_tuned and benchmark take device pointers as plain integers.  There is
no plan and nothing to prepare; timings are ADDED to a running total, as in smfft_amd.api.  Refusals are raised before a device is
touched.  There is no CPU fallback: a missing library raises on first call.
"""
import ctypes

import numpy as np

from . import _addon
from ._rows import check_tensor as _check_tensor
from ._rows import host_round_trip as _host_round_trip

SIZES = (256, 512, 1024, 2048, 4096)          # the inner transform lengths M = n / 2
LENGTHS = (512, 1024, 2048, 4096, 8192)       # the row lengths n
QUADRATURE, ANALYTIC, ENVELOPE = 0, 1, 2      # SMFFT_HILBERT_QUADRATURE, _ANALYTIC, _ENVELOPE
KINDS = (QUADRATURE, ANALYTIC, ENVELOPE)

_vp, _i, _ll, _dp = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.POINTER(ctypes.c_double)
_HEAD = [_vp, _vp, _i, _ll, _i]               # d_in, d_out, n, batch, kind
# name -> (restype, argtypes), exactly the declarations of include/smfft_hilbert.h (tests/test_sm_hilbert_cpu.py compares them)
SIGS = {
    "smfft_hilbert_fft_size": (_i, [_i]),
    "smfft_hilbert_launch": (_i, _HEAD + [_vp]),
    "smfft_hilbert_launch_tuned": (_i, _HEAD + [_vp, _i]),
    "smfft_hilbert_benchmark": (_i, _HEAD + [_dp]),
}

LIB_PATH, load, lib = _addon.loader("libsmfft_hilbert.so", "SMFFT_HILBERT_LIB", __name__, SIGS)
_lib = None


def _check(n, kind):
    n, kind = int(n), int(kind)
    if n not in LENGTHS:
        raise ValueError(f"smfft_amd.hilbert serves rows of n in {LENGTHS} points, not n = {n}")
    if kind not in KINDS:
        raise ValueError(f"smfft_amd.hilbert serves kinds 0 (quadrature), 1 (analytic) and 2 (envelope), not kind = {kind}")
    return n, kind


def fft_size(n):
    """M = n / 2, the length of the kernel's complex transforms (smfft_hilbert_fft_size)"""
    return lib().smfft_hilbert_fft_size(_check(n, 0)[0])


def launch_ptr(d_in, d_out, n, batch, kind=QUADRATURE, stream=0):
    """batch rows of n float32 points from d_in, the output of `kind` to d_out (device pointers; d_out == d_in is allowed for kinds
    0 and 2; kind 1 writes batch * n complex64), launch only (no events, no sync) (smfft_hilbert_launch)"""
    rc = lib().smfft_hilbert_launch(d_in, d_out, n, batch, kind, stream)
    if rc != 0:
        raise RuntimeError(f"smfft_hilbert_launch(n={n}, batch={batch}, kind={kind}) -> {rc}")


def launch_tuned(d_in, d_out, n, batch, grid, kind=QUADRATURE, stream=0):
    """the same launch on `grid` workgroups (>= 1); the result does not depend on it (smfft_hilbert_launch_tuned)"""
    rc = lib().smfft_hilbert_launch_tuned(d_in, d_out, n, batch, kind, stream, grid)
    if rc != 0:
        raise RuntimeError(f"smfft_hilbert_launch_tuned(n={n}, batch={batch}, kind={kind}, grid={grid}) -> {rc}")


def benchmark(d_in, d_out, n, batch, kind=QUADRATURE):
    """One launch on the null stream, timed with events; synchronous.  Returns (status, elapsed_ms)."""
    t = ctypes.c_double(0.0)
    rc = lib().smfft_hilbert_benchmark(d_in, d_out, n, batch, kind, ctypes.byref(t))
    return rc, t.value


def launch(x, out=None, kind=QUADRATURE, stream=None):
    """x: a contiguous float32 torch tensor on the device, rows on the last axis; out: a contiguous tensor of the same shape -- float32,
    or complex64 for the analytic kind --, x itself (in place: kinds 0 and 2), or None for a new one.  Enqueues one launch on `stream`
    (a hipStream_t as an integer; None = torch's current stream of x's device) and returns out; nothing is synchronised"""
    import torch
    x = _check_tensor(x, "x", torch.float32)
    n, kind = _check(x.shape[-1], kind)                                  # (refuses before anything touches a device)
    out_dtype = torch.complex64 if kind == ANALYTIC else torch.float32
    if out is not None and (_check_tensor(out, "out", out_dtype).shape != x.shape or out.device != x.device):
        raise ValueError(f"out must have x's shape and device: {tuple(out.shape)} on {out.device} against {tuple(x.shape)} on {x.device}")
    if not x.is_cuda:
        raise ValueError("smfft_amd.hilbert.launch takes tensors on the device; host arrays go through hilbert() / analytic() / "
                         "envelope().  There is no CPU fallback")
    handle = lib()
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    if stream is None:
        stream = torch.cuda.current_stream(x.device).cuda_stream
    batch = x.numel() // n
    with torch.cuda.device(x.device):
        rc = handle.smfft_hilbert_launch(x.data_ptr(), out.data_ptr(), n, batch, kind, stream)
    if rc != 0:
        raise RuntimeError(f"smfft_hilbert_launch(n={n}, batch={batch}, kind={kind}) -> {rc}")
    return out


def _transform(x, kind):
    if type(x).__module__.split(".")[0] == "torch":                 # a tensor, without importing torch for host arrays
        import torch
        if x.is_cuda:
            return launch(x, None, kind)
        return torch.from_numpy(_transform(x.numpy(), kind))
    x = np.asarray(x)
    if np.iscomplexobj(x):
        raise TypeError("smfft_amd.hilbert takes real rows")
    if x.ndim < 1:
        raise ValueError("x must have at least one axis")
    n, kind = _check(x.shape[-1], kind)                                  # (refuses before anything touches a device)
    shape = x.shape
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, n)
    batch = x.shape[0]
    handle = lib()
    return _host_round_trip(x, np.complex64 if kind == ANALYTIC else np.float32, lambda din, dout: handle.smfft_hilbert_launch(din, dout, n, batch, kind, None),
                            f"hilbert(n={n}, batch={batch}, kind={kind})").reshape(shape)


def hilbert(x):
    """the Hilbert transform H(x) along the last axis (scipy.signal.hilbert(x).imag).  x: a contiguous float32 torch tensor on the
    device -> a new tensor there, from one launch on torch's current stream; or a host array / CPU tensor of any real dtype -> float32
    of the same shape through a host round trip (upload, one launch, download)"""
    return _transform(x, QUADRATURE)


def analytic(x):
    """the analytic signal x + i H(x) along the last axis, complex64; its real part is x (as float32) to the bit; x as in hilbert()"""
    return _transform(x, ANALYTIC)


def envelope(x):
    """the envelope sqrt(x^2 + H(x)^2) along the last axis, float32; x as in hilbert()"""
    return _transform(x, ENVELOPE)

"""ctypes mirror of include/smfft_dct.h: batched DCT-II / DCT-III / DST-II / DST-III of real rows of n = 512 ... 8192 points (powers of
two) in one kernel (libsmfft_dct.so: the permuted row in the two lanes of one complex transform of M = n / 2 points on the register
engine, a Hermitian split and a quarter-wave twiddle).  float32 in, float32 out, un-normalised -- scipy.fft's norm=None:

    dct(x, 2)[k] = 2 sum_j x[j] cos(pi k (2j+1) / (2n))                       = scipy.fft.dct(x, 2)
    dct(X, 3)[j] = X[0] + 2 sum_{k>=1} X[k] cos(pi k (2j+1) / (2n))            = scipy.fft.dct(X, 3);  dct(dct(x, 2), 3) = 2n x
    dst(x, 2)[k] = 2 sum_j x[j] sin(pi (k+1)(2j+1) / (2n))                     = scipy.fft.dst(x, 2)
    dst(X, 3)[j] = (-1)^j X[n-1] + 2 sum_{k<n-1} X[k] sin(pi (k+1)(2j+1) / (2n)) = scipy.fft.dst(X, 3);  dst(dst(x, 2), 3) = 2n x

The library is loaded on first use, so that `import smfft_amd` behaves the same whether it was built or not.  launch / dct / dst take
tensors; launch_ptr, launch_tuned and benchmark take device pointers as plain integers.  There is no plan and nothing to prepare;
timings are ADDED to a running total, as in smfft_amd.api.  Refusals are raised before a device is touched.  There is no CPU
fallback: a missing library raises on first call.
"""
import ctypes

import numpy as np

from . import _addon
from ._rows import check_tensor as _check_tensor
from ._rows import host_round_trip as _host_round_trip

SIZES = (256, 512, 1024, 2048, 4096)          # the inner transform lengths M = n / 2
LENGTHS = (512, 1024, 2048, 4096, 8192)       # the row lengths n
TYPES = (2, 3)
_type_of = type                               # (the functions below take `type` as an argument, scipy's name for it)

_vp, _i, _ll, _dp = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.POINTER(ctypes.c_double)
_HEAD = [_vp, _vp, _i, _ll, _i, _i]           # d_in, d_out, n, batch, type, sine
# name -> (restype, argtypes), exactly the declarations of include/smfft_dct.h (tests/test_sm_dct_cpu.py compares them)
SIGS = {
    "smfft_dct_fft_size": (_i, [_i]),
    "smfft_dct_launch": (_i, _HEAD + [_vp]),
    "smfft_dct_launch_tuned": (_i, _HEAD + [_vp, _i]),
    "smfft_dct_benchmark": (_i, _HEAD + [_dp]),
}

LIB_PATH, load, lib = _addon.loader("libsmfft_dct.so", "SMFFT_DCT_LIB", __name__, SIGS)
_lib = None


def _check(n, type):
    n, type = int(n), int(type)
    if n not in LENGTHS:
        raise ValueError(f"smfft_amd.dct serves rows of n in {LENGTHS} points, not n = {n}")
    if type not in TYPES:
        raise ValueError(f"smfft_amd.dct serves types 2 and 3, not type = {type}")
    return n, type


def fft_size(n):
    """M = n / 2, the length of the kernel's complex transform (smfft_dct_fft_size)"""
    return lib().smfft_dct_fft_size(_check(n, 2)[0])


def launch_ptr(d_in, d_out, n, batch, type=2, sine=False, stream=0):
    """batch transforms of float32 rows of n points from d_in to d_out (device pointers; d_out == d_in is allowed), launch only (no
    events, no sync) (smfft_dct_launch)"""
    rc = lib().smfft_dct_launch(d_in, d_out, n, batch, type, int(bool(sine)), stream)
    if rc != 0:
        raise RuntimeError(f"smfft_dct_launch(n={n}, batch={batch}, type={type}, sine={bool(sine)}) -> {rc}")


def launch_tuned(d_in, d_out, n, batch, grid, type=2, sine=False, stream=0):
    """the same launch on `grid` workgroups (>= 1); the result does not depend on it (smfft_dct_launch_tuned)"""
    rc = lib().smfft_dct_launch_tuned(d_in, d_out, n, batch, type, int(bool(sine)), stream, grid)
    if rc != 0:
        raise RuntimeError(f"smfft_dct_launch_tuned(n={n}, batch={batch}, type={type}, sine={bool(sine)}, grid={grid}) -> {rc}")


def benchmark(d_in, d_out, n, batch, type=2, sine=False):
    """One launch on the null stream, timed with events; synchronous.  Returns (status, elapsed_ms)."""
    t = ctypes.c_double(0.0)
    rc = lib().smfft_dct_benchmark(d_in, d_out, n, batch, type, int(bool(sine)), ctypes.byref(t))
    return rc, t.value


def launch(x, out=None, type=2, sine=False, stream=None):
    """x: a contiguous float32 torch tensor on the device, rows on the last axis; out: such a tensor of the same shape, x itself (in
    place), or None for a new one.  Enqueues one launch on `stream` (a hipStream_t as an integer; None = torch's current stream of x's
    device) and returns out; nothing is synchronised"""
    x = _check_tensor(x, "x")
    n, type = _check(x.shape[-1], type)                                  # (refuses before anything touches a device)
    if out is not None and (_check_tensor(out, "out").shape != x.shape or out.device != x.device):
        raise ValueError(f"out must have x's shape and device: {tuple(out.shape)} on {out.device} against {tuple(x.shape)} on {x.device}")
    if not x.is_cuda:
        raise ValueError("smfft_amd.dct.launch takes tensors on the device; host arrays go through dct() / dst().  There is no CPU fallback")
    import torch
    handle = lib()
    if out is None:
        out = torch.empty_like(x)
    if stream is None:
        stream = torch.cuda.current_stream(x.device).cuda_stream
    batch = x.numel() // n
    with torch.cuda.device(x.device):
        rc = handle.smfft_dct_launch(x.data_ptr(), out.data_ptr(), n, batch, type, int(bool(sine)), stream)
    if rc != 0:
        raise RuntimeError(f"smfft_dct_launch(n={n}, batch={batch}, type={type}, sine={bool(sine)}) -> {rc}")
    return out


def _transform(x, type, sine):
    if _type_of(x).__module__.split(".")[0] == "torch":             # a tensor, without importing torch for host arrays
        import torch
        if x.is_cuda:
            return launch(x, None, type, sine)
        return torch.from_numpy(_transform(x.numpy(), type, sine))
    x = np.asarray(x)
    if np.iscomplexobj(x):
        raise TypeError("smfft_amd.dct takes real rows")
    if x.ndim < 1:
        raise ValueError("x must have at least one axis")
    n, type = _check(x.shape[-1], type)                                  # (refuses before anything touches a device)
    shape = x.shape
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, n)
    batch = x.shape[0]
    handle = lib()
    return _host_round_trip(x, np.float32, lambda din, dout: handle.smfft_dct_launch(din, dout, n, batch, type, int(bool(sine)), None),
                            f"dct(n={n}, batch={batch}, type={type}, sine={bool(sine)})").reshape(shape)


def dct(x, type=2):
    """the DCT of type 2 or 3 along the last axis.  x: a contiguous float32 torch tensor on the device -> a new tensor there, from one
    launch on torch's current stream; or a host array / CPU tensor of any real dtype -> float32 of the same shape through a host
    round trip (upload, one launch, download)"""
    return _transform(x, type, False)


def dst(x, type=2):
    """the DST of type 2 or 3 along the last axis; x as in dct()"""
    return _transform(x, type, True)

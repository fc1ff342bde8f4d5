"""ctypes mirror of include/smfft_stft.h: the batched short-time Fourier transform of real signals in frames of n = 512 ... 8192 samples
(powers of two) at any hop, as complex spectra or as power, and the inverse transform of such frames, each in one kernel
(libsmfft_stft.so: consecutive pairs of windowed samples in the two lanes of one complex transform of M = n / 2 points on the register
engine, the Hermitian split and the radix-2 merge behind it or in front of it; the frames are read from the signal itself).  float32
in, complex64 or float32 out:

    stft(s, n, hop, w)[c, f, k] = sum_{j<n} w[j] s[c, f hop + j] exp(-2 pi i jk / n),  k <= n / 2   = torch.stft(...).transpose(-1, -2)
    spectrogram(s, n, hop, w)   = |stft|^2, from a kernel of its own
    istft_frames(X, w)[..., j]  = w[j] irfft_n(X)[j]                                               = torch.fft.irfft(X, n) * w
    istft(X, hop, w)            = overlap_add(istft_frames(X, w), hop, w)                           = torch.istft(X.transpose(-1, -2), ...)

The library is loaded on first use, so that `import smfft_amd` behaves the same whether it was built or not.  The functions take
tensors on the device; the *_ptr and *_benchmark forms take device pointers as plain integers.  There is no plan and nothing to
prepare; timings are ADDED to a running total, as in smfft_amd.api.  Refusals are raised before a device is touched.  There is no CPU
fallback: a missing library raises on first call.
"""
import ctypes

import numpy as np

from . import _addon
from ._rows import check_tensor as _check_tensor

SIZES = (256, 512, 1024, 2048, 4096)          # the inner transform lengths M = n / 2
LENGTHS = (512, 1024, 2048, 4096, 8192)       # the frame lengths n

_vp, _i, _ll, _dp = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.POINTER(ctypes.c_double)
_STFT = [_vp, _vp, _vp, _i, _ll, _ll, _ll, _ll, _i]   # d_in, d_out, d_window, n, streams, frames, hop, stream_stride, kind
_ISTFT = [_vp, _vp, _vp, _i, _ll]             # d_in, d_out, d_window, n, batch
# name -> (restype, argtypes), exactly the declarations of include/smfft_stft.h (tests/test_sm_stft_cpu.py compares them)
SIGS = {
    "smfft_stft_fft_size": (_i, [_i]),
    "smfft_stft_frames": (_ll, [_ll, _i, _ll]),
    "smfft_stft_launch": (_i, _STFT + [_vp]),
    "smfft_stft_launch_tuned": (_i, _STFT + [_vp, _i]),
    "smfft_stft_benchmark": (_i, _STFT + [_dp]),
    "smfft_istft_launch": (_i, _ISTFT + [_vp]),
    "smfft_istft_launch_tuned": (_i, _ISTFT + [_vp, _i]),
    "smfft_istft_benchmark": (_i, _ISTFT + [_dp]),
}

LIB_PATH, load, lib = _addon.loader("libsmfft_stft.so", "SMFFT_STFT_LIB", __name__, SIGS)
_lib = None


def _check(n):
    n = int(n)
    if n not in LENGTHS:
        raise ValueError(f"smfft_amd.stft serves n in {LENGTHS}, not {n}")
    return n


def _raise(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} -> {rc}")


def fft_size(n):
    """M = n / 2, the length of the kernels' complex transform (smfft_stft_fft_size)"""
    return lib().smfft_stft_fft_size(_check(n))


def frames(L, n, hop):
    """the whole frames of n samples at hop in L samples: 1 + (L - n) // hop, 0 for L < n (smfft_stft_frames)"""
    count = lib().smfft_stft_frames(int(L), _check(n), int(hop))
    if count < 0:
        raise ValueError(f"smfft_stft_frames(L={L}, n={n}, hop={hop}) -> {count}")
    return count


# ---- device pointers -------------------------------------------------------------------------------------------------------------------
def launch_ptr(d_in, d_out, d_window, n, streams, frames, hop, stream_stride, power=False, stream=0, grid=None):
    """streams * frames transforms: frame (c, f) reads d_in[c stream_stride + f hop ... + n) and writes n / 2 + 1 complex64 (power:
    float32 powers) at element (c frames + f)(n / 2 + 1) of d_out; d_window: n floats or None (smfft_stft_launch; grid: on that many
    workgroups, smfft_stft_launch_tuned)"""
    if grid is None:
        rc = lib().smfft_stft_launch(d_in, d_out, d_window, n, streams, frames, hop, stream_stride, int(bool(power)), stream)
    else:
        rc = lib().smfft_stft_launch_tuned(d_in, d_out, d_window, n, streams, frames, hop, stream_stride, int(bool(power)), stream, grid)
    _raise(rc, f"smfft_stft_launch(n={n}, streams={streams}, frames={frames}, hop={hop}, stream_stride={stream_stride}, power={bool(power)}, grid={grid})")


def istft_ptr(d_in, d_out, d_window, n, batch, stream=0, grid=None):
    """batch inverse transforms: rows of n / 2 + 1 complex64 at d_in, rows of n windowed samples at d_out (smfft_istft_launch; grid:
    smfft_istft_launch_tuned)"""
    if grid is None:
        rc = lib().smfft_istft_launch(d_in, d_out, d_window, n, batch, stream)
    else:
        rc = lib().smfft_istft_launch_tuned(d_in, d_out, d_window, n, batch, stream, grid)
    _raise(rc, f"smfft_istft_launch(n={n}, batch={batch}, grid={grid})")


def stft_benchmark(d_in, d_out, d_window, n, streams, frames, hop, stream_stride, power=False):
    """One launch on the null stream, timed with events; synchronous.  Returns (status, elapsed_ms)."""
    t = ctypes.c_double(0.0)
    rc = lib().smfft_stft_benchmark(d_in, d_out, d_window, n, streams, frames, hop, stream_stride, int(bool(power)), ctypes.byref(t))
    return rc, t.value


def istft_benchmark(d_in, d_out, d_window, n, batch):
    t = ctypes.c_double(0.0)
    rc = lib().smfft_istft_benchmark(d_in, d_out, d_window, n, batch, ctypes.byref(t))
    return rc, t.value


# ---- tensors ---------------------------------------------------------------------------------------------------------------------------
def _check_window(window, n, x):
    if window is None:
        return None
    w = _check_tensor(window, "window")
    if w.shape != (n,):
        raise ValueError(f"window must hold n = {n} floats, not {tuple(w.shape)}")
    if w.device != x.device:
        raise ValueError(f"window must be on the signal's device: {w.device} against {x.device}")
    return w


def _on_device(x, what):
    if not x.is_cuda:
        raise ValueError(f"smfft_amd.stft.{what} takes tensors on the device.  There is no CPU fallback")


def _stream(x, stream):
    import torch
    return torch.cuda.current_stream(x.device).cuda_stream if stream is None else stream


def launch(signal, n, hop, window=None, power=False, stream=None):
    """signal: (streams, L) or (L,) contiguous float32 on the device, L >= n -> (streams, frames, n / 2 + 1) complex64 (power:
    float32), frames = 1 + (L - n) // hop, frame f of stream c from signal[c, f hop ... f hop + n) in one launch that reads every
    sample from the signal itself.  Enqueues on `stream` (a hipStream_t as an integer; None = torch's current stream of the signal's
    device); nothing is synchronised"""
    s = _check_tensor(signal, "signal")
    n, hop = _check(n), int(hop)
    if s.ndim > 2 or s.shape[-1] < n:
        raise ValueError(f"signal must be (streams, L) or (L,) with L >= n = {n}, not {tuple(s.shape)}")
    if hop < 1:
        raise ValueError(f"hop must be at least 1, not {hop}")
    w = _check_window(window, n, s)
    _on_device(s, "launch")
    import torch
    handle = lib()
    L = s.shape[-1]
    C = s.numel() // L
    F = 1 + (L - n) // hop
    out = torch.empty((C, F, n // 2 + 1), dtype=torch.float32 if power else torch.complex64, device=s.device)
    with torch.cuda.device(s.device):
        rc = handle.smfft_stft_launch(s.data_ptr(), out.data_ptr(), None if w is None else w.data_ptr(), n, C, F, hop, L, int(bool(power)), _stream(s, stream))
    _raise(rc, f"smfft_stft_launch(n={n}, streams={C}, frames={F}, hop={hop}, stream_stride={L}, power={bool(power)})")
    return out


def stft(signal, n, hop, window=None, power=False, center=False):
    """the short-time Fourier transform of signal (streams, L) or (L,) -> (streams, frames, n / 2 + 1), one launch.  window: n float32
    on the same device, or None for all ones.  center=True reflect-pads n / 2 samples on each side first, in plain torch (one padded
    copy of the signal), and then equals torch.stft(center=True, pad_mode="reflect") transposed"""
    if center:
        s = _check_tensor(signal, "signal")
        n = _check(n)
        if s.ndim > 2 or s.shape[-1] <= n // 2:
            raise ValueError(f"signal must be (streams, L) or (L,) with L > n / 2 = {n // 2} for reflect padding, not {tuple(s.shape)}")
        import torch
        signal = torch.nn.functional.pad(s.reshape(-1, s.shape[-1]).unsqueeze(0), (n // 2, n // 2), mode="reflect").squeeze(0).contiguous()
    return launch(signal, n, hop, window, power)


def spectrogram(signal, n, hop, window=None, center=False):
    """|stft|^2 as float32 (streams, frames, n / 2 + 1), from the power kernel: the complex spectrum never reaches memory"""
    return stft(signal, n, hop, window, True, center)


def istft_frames(X, window=None, stream=None):
    """the inverse transform of rows of n / 2 + 1 complex64 bins on the last axis of a contiguous tensor on the device -> (..., n)
    windowed float32 samples, one launch; overlap_add() sums them"""
    import torch
    X = _check_tensor(X, "X", torch.complex64)
    if X.shape[-1] < 2:
        raise ValueError(f"rows of n / 2 + 1 bins, not {X.shape[-1]}")
    n = _check(2 * (X.shape[-1] - 1))
    w = _check_window(window, n, X)
    _on_device(X, "istft_frames")
    handle = lib()
    out = torch.empty(X.shape[:-1] + (n,), dtype=torch.float32, device=X.device)
    rows = X.numel() // (n // 2 + 1)
    with torch.cuda.device(X.device):
        rc = handle.smfft_istft_launch(X.data_ptr(), out.data_ptr(), None if w is None else w.data_ptr(), n, rows, _stream(X, stream))
    _raise(rc, f"smfft_istft_launch(n={n}, batch={rows})")
    return out


def overlap_add(y, hop, window=None, length=None, center=False):
    """(..., F, n) -> (..., (F - 1) hop + n), cut or zero-padded to `length`: frame f added at offset f hop.  Plain torch operations
    (a fold), not a kernel of this library: the inverse kernel writes every frame once and adds nothing.  With a window the sum is
    divided by the sum of the squared window at the same offsets, and a ValueError is raised where that envelope is below 1e-11,
    which is torch.istft's rule.  center=True starts n / 2 samples into the sum (behind the padding of
    stft(center=True)) and, without a `length`, ends n / 2 samples before its end, in front of that check, as torch.istft does"""
    import torch
    hop = int(hop)
    F, n = y.shape[-2], y.shape[-1]
    if hop < 1:
        raise ValueError(f"hop must be at least 1, not {hop}")
    total = (F - 1) * hop + n
    lead = y.shape[:-2]

    def fold(frames_):                           # (B, F, n) -> (B, total)
        return torch.nn.functional.fold(frames_.transpose(1, 2), (1, total), (1, n), stride=(1, hop)).reshape(frames_.shape[0], total)
    # the range of the sum that is returned: torch.istft's (start behind the padding, end at `length` where one is given)
    start = n // 2 if center else 0
    end = min(total, start + length) if length is not None else total - start
    out = fold(y.reshape(-1, F, n))[:, start:end]
    if window is not None:
        env = fold((window.to(y.dtype) ** 2).expand(1, F, n))[0, start:end]
        if float(env.abs().min()) < 1e-11:
            raise ValueError("the window's overlap-add envelope falls below 1e-11")
        out = out / env
    if length is not None and out.shape[1] < length:
        out = torch.nn.functional.pad(out, (0, length - out.shape[1]))
    return out.reshape(lead + (out.shape[1],))


def istft(X, hop, window, length=None, center=False):
    """overlap_add(istft_frames(X, window), hop, window, length, center): the signal back from the frames of stft() with the same
    window, hop and center, wherever the window's envelope is not zero (a window that starts at zero, as hann() does, needs
    center=True or frames that start before the samples wanted: torch.istft's rule)"""
    return overlap_add(istft_frames(X, window), hop, window, length, center)


def hann(n, device=None):
    """the periodic Hann window 0.5 - 0.5 cos(2 pi j / n), j < n, computed in fp64 and rounded once"""
    import torch
    n = _check(n)
    w = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n, dtype=np.float64) / n)).astype(np.float32)
    return torch.from_numpy(w).to(device) if device is not None else torch.from_numpy(w)

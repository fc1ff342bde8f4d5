"""ctypes mirror of include/smfft_welch.h: Welch power spectra and cross spectra of real signals (libsmfft_welch.so: the frames of
smfft_amd.stft -- n = 512 ... 8192 samples, powers of two, at any hop -- summed over T consecutive frames inside the kernel, as |X|^2 of
one signal or as conj(X) Y of two; the frames' spectra never reach memory).  float32 in, float32 or complex64 out:

    dynamic_spectrum(s, n, hop, T, w)[c, g, k] = sum_{t<T} |stft(s, n, hop, w)[c, g T + t, k]|^2        raw sums, one launch
    welch(x, fs, w, n, hop)                    = scipy.signal.welch(x, fs, w, n, n - hop, detrend=False)[1]
    csd(x, y, fs, w, n, hop)                   = scipy.signal.csd(x, y, fs, w, n, n - hop, detrend=False)[1]
    coherence(x, y, w, n, hop)                 = scipy.signal.coherence(x, y, 1.0, w, n, n - hop, detrend=False)[1]

The library is loaded on first use, so that `import smfft_amd` behaves the same whether it was built or not.  The functions take
tensors on the device; the *_ptr and *_benchmark forms take device pointers as plain integers.  There is no plan and nothing to
prepare; timings are ADDED to a running total, as in smfft_amd.api.  Refusals are raised before a device is touched.  There is no CPU
fallback: a missing library raises on first call.
"""
import ctypes

from . import _addon
from ._rows import check_tensor as _check_tensor
from .stft import hann  # noqa: F401  (the periodic Hann window, for callers of this module)

SIZES = (256, 512, 1024, 2048, 4096)          # the inner transform lengths M = n / 2
LENGTHS = (512, 1024, 2048, 4096, 8192)       # the frame lengths n

_vp, _i, _ll, _dp = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.POINTER(ctypes.c_double)
_WELCH = [_vp, _vp, _vp, _i, _ll, _ll, _ll, _ll, _ll]            # d_in, d_out, d_window, n, streams, groups, T, hop, stream_stride
_CSD = [_vp, _vp, _vp, _vp, _i, _ll, _ll, _ll, _ll, _ll, _ll]    # d_x, d_y, d_out, d_window, n, streams, groups, T, hop, x_stride, y_stride
# name -> (restype, argtypes), exactly the declarations of include/smfft_welch.h (tests/test_sm_welch_cpu.py compares them)
SIGS = {
    "smfft_welch_fft_size": (_i, [_i]),
    "smfft_welch_groups": (_ll, [_ll, _i, _ll, _ll]),
    "smfft_welch_launch": (_i, _WELCH + [_vp]),
    "smfft_welch_launch_tuned": (_i, _WELCH + [_vp, _i]),
    "smfft_welch_benchmark": (_i, _WELCH + [_dp]),
    "smfft_csd_launch": (_i, _CSD + [_vp]),
    "smfft_csd_launch_tuned": (_i, _CSD + [_vp, _i]),
    "smfft_csd_benchmark": (_i, _CSD + [_dp]),
}

LIB_PATH, load, lib = _addon.loader("libsmfft_welch.so", "SMFFT_WELCH_LIB", __name__, SIGS)
_lib = None

# the default T of the helpers (default_T): as many (stream, group) slots as sixteen fillings of the chip -- 256 compute units, 2 workgroups
# on each, 4096 / M slots per workgroup.  By measurement (tools/ab_welch.py, profiles/r27_welch_ab.txt): with two fillings, the first
# rule, the auto kernel took up to 1.33 times as long as at T = 8 (the last, partly filled round of workgroups weighs more the fewer
# rounds there are), and the output of T = 8 is already 1 / 8 of the spectrogram's
_COMPUTE_UNITS, _WORKGROUPS_PER_CU, _FILLINGS = 256, 2, 16


def _check(n):
    n = int(n)
    if n not in LENGTHS:
        raise ValueError(f"smfft_amd.welch serves n in {LENGTHS}, not {n}")
    return n


def _raise(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} -> {rc}")


def fft_size(n):
    """M = n / 2, the length of the kernels' complex transform (smfft_welch_fft_size)"""
    return lib().smfft_welch_fft_size(_check(n))


def groups(L, n, hop, T):
    """the whole groups of T frames of n samples at hop in L samples: (1 + (L - n) // hop) // T, 0 for L < n (smfft_welch_groups)"""
    count = lib().smfft_welch_groups(int(L), _check(n), int(hop), int(T))
    if count < 0:
        raise ValueError(f"smfft_welch_groups(L={L}, n={n}, hop={hop}, T={T}) -> {count}")
    return count


def default_T(streams, frames, n):
    """the frames per group that the helpers sum in the kernel when none is given: the largest T with streams * (frames // T) >=
    16 * 256 compute units * 2 workgroups * (8192 / n) slots, at least 1 -- longer sums store less, shorter ones fill the chip"""
    slots = _FILLINGS * _COMPUTE_UNITS * _WORKGROUPS_PER_CU * (8192 // _check(n))
    want = -(-slots // max(int(streams), 1))            # groups per stream
    return max(1, int(frames) // want)


# ---- device pointers -------------------------------------------------------------------------------------------------------------------
def launch_ptr(d_in, d_out, d_window, n, streams, groups, T, hop, stream_stride, stream=0, grid=None):
    """streams * groups auto spectra: group (c, g) sums the powers of frames g T ... g T + T - 1 of stream c, frame f at
    d_in[c stream_stride + f hop ... + n), into n / 2 + 1 float32 at element (c groups + g)(n / 2 + 1) of d_out; d_window: n floats or
    None (smfft_welch_launch; grid: on that many workgroups, smfft_welch_launch_tuned)"""
    if grid is None:
        rc = lib().smfft_welch_launch(d_in, d_out, d_window, n, streams, groups, T, hop, stream_stride, stream)
    else:
        rc = lib().smfft_welch_launch_tuned(d_in, d_out, d_window, n, streams, groups, T, hop, stream_stride, stream, grid)
    _raise(rc, f"smfft_welch_launch(n={n}, streams={streams}, groups={groups}, T={T}, hop={hop}, stream_stride={stream_stride}, grid={grid})")


def csd_ptr(d_x, d_y, d_out, d_window, n, streams, groups, T, hop, x_stride, y_stride, stream=0, grid=None):
    """streams * groups cross spectra: the sums of conj(X) Y over the same groups of d_x and d_y into n / 2 + 1 complex64 each;
    y_stride = 0: one reference stream for all streams of x (smfft_csd_launch; grid: smfft_csd_launch_tuned)"""
    if grid is None:
        rc = lib().smfft_csd_launch(d_x, d_y, d_out, d_window, n, streams, groups, T, hop, x_stride, y_stride, stream)
    else:
        rc = lib().smfft_csd_launch_tuned(d_x, d_y, d_out, d_window, n, streams, groups, T, hop, x_stride, y_stride, stream, grid)
    _raise(rc, f"smfft_csd_launch(n={n}, streams={streams}, groups={groups}, T={T}, hop={hop}, x_stride={x_stride}, y_stride={y_stride}, grid={grid})")


def welch_benchmark(d_in, d_out, d_window, n, streams, groups, T, hop, stream_stride):
    """One launch on the null stream, timed with events; synchronous.  Returns (status, elapsed_ms)."""
    t = ctypes.c_double(0.0)
    rc = lib().smfft_welch_benchmark(d_in, d_out, d_window, n, streams, groups, T, hop, stream_stride, ctypes.byref(t))
    return rc, t.value


def csd_benchmark(d_x, d_y, d_out, d_window, n, streams, groups, T, hop, x_stride, y_stride):
    t = ctypes.c_double(0.0)
    rc = lib().smfft_csd_benchmark(d_x, d_y, d_out, d_window, n, streams, groups, T, hop, x_stride, y_stride, ctypes.byref(t))
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


def _check_signal(signal, what, n):
    s = _check_tensor(signal, what)
    if s.ndim > 2 or s.shape[-1] < n:
        raise ValueError(f"{what} must be (streams, L) or (L,) with L >= n = {n}, not {tuple(s.shape)}")
    return s


def _check_counts(hop, T):
    hop, T = int(hop), int(T)
    if hop < 1:
        raise ValueError(f"hop must be at least 1, not {hop}")
    if T < 1:
        raise ValueError(f"T must be at least 1, not {T}")
    return hop, T


def _on_device(x, what):
    if not x.is_cuda:
        raise ValueError(f"smfft_amd.welch.{what} takes tensors on the device.  There is no CPU fallback")


def _stream(x, stream):
    import torch
    return torch.cuda.current_stream(x.device).cuda_stream if stream is None else stream


def _pair(x, y, n):
    """x: (streams, L) or (L,), y: the same shape, or (L,) / (1, L) as the one reference of all streams -> (x, y, streams, L, y_stride)"""
    x, y = _check_signal(x, "x", n), _check_signal(y, "y", n)
    L = x.shape[-1]
    C = x.numel() // L
    if y.shape[-1] != L or y.numel() not in (L, x.numel()) or y.device != x.device:
        raise ValueError(f"y must have x's shape {tuple(x.shape)} or be one stream of {L} samples on x's device, not {tuple(y.shape)} on {y.device}")
    return x, y, C, L, (L if y.numel() == x.numel() and C > 1 else 0)


def _auto(s, w, n, C, L, first, G, T, hop, stream):
    """one launch: G groups of T frames per stream, from frame `first` on, through a pointer offset"""
    import torch
    out = torch.empty((C, G, n // 2 + 1), dtype=torch.float32, device=s.device)
    with torch.cuda.device(s.device):
        rc = lib().smfft_welch_launch(s.data_ptr() + 4 * first * hop, out.data_ptr(), None if w is None else w.data_ptr(), n, C, G, T, hop, L, _stream(s, stream))
    _raise(rc, f"smfft_welch_launch(n={n}, streams={C}, groups={G}, T={T}, hop={hop}, stream_stride={L})")
    return out


def _cross(x, y, w, n, C, L, y_stride, first, G, T, hop, stream):
    import torch
    out = torch.empty((C, G, n // 2 + 1), dtype=torch.complex64, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib().smfft_csd_launch(x.data_ptr() + 4 * first * hop, y.data_ptr() + 4 * first * hop, out.data_ptr(), None if w is None else w.data_ptr(),
                                    n, C, G, T, hop, L, y_stride, _stream(x, stream))
    _raise(rc, f"smfft_csd_launch(n={n}, streams={C}, groups={G}, T={T}, hop={hop}, x_stride={L}, y_stride={y_stride})")
    return out


def launch(signal, n, hop, T, window=None, stream=None):
    """signal: (streams, L) or (L,) contiguous float32 on the device, L >= n -> (streams, groups, n / 2 + 1) float32,
    groups = frames // T of frames = 1 + (L - n) // hop: the sums of the powers of T consecutive frames, in one launch that reads every
    sample from the signal itself; the frames behind the last whole group are left out.  Enqueues on `stream` (a hipStream_t as an
    integer; None = torch's current stream of the signal's device); nothing is synchronised"""
    n = _check(n)
    s = _check_signal(signal, "signal", n)
    hop, T = _check_counts(hop, T)
    w = _check_window(window, n, s)
    _on_device(s, "launch")
    L = s.shape[-1]
    return _auto(s, w, n, s.numel() // L, L, 0, (1 + (L - n) // hop) // T, T, hop, stream)


def csd_launch(x, y, n, hop, T, window=None, stream=None):
    """x: (streams, L) or (L,), y: x's shape or one stream of L samples (the reference of every stream of x) ->
    (streams, groups, n / 2 + 1) complex64: the sums of conj(X) Y over T consecutive frames, in one launch"""
    n = _check(n)
    x, y, C, L, y_stride = _pair(x, y, n)
    hop, T = _check_counts(hop, T)
    w = _check_window(window, n, x)
    _on_device(x, "csd_launch")
    return _cross(x, y, w, n, C, L, y_stride, 0, (1 + (L - n) // hop) // T, T, hop, stream)


def dynamic_spectrum(signal, n, hop, T, window=None):
    """(streams, groups, n / 2 + 1) raw sums of the powers of T consecutive frames: a spectrogram integrated in the kernel"""
    return launch(signal, n, hop, T, window)


def _all_frames(F, T, one):
    """the sum over all F frames of the partial spectra of one(first frame, groups, frames per group): one launch of F // T groups of
    T and, where T does not divide F, a second one of one group of the F - (F // T) T frames left"""
    G = F // T
    total = one(0, G, T).sum(dim=1) if G else None
    if F > G * T:
        rest = one(G * T, 1, F - G * T)[:, 0]
        total = rest if total is None else total + rest
    return total


def _scale(n, F, w, fs, scaling, device):
    """(n / 2 + 1,) float64 on the device: scipy's factors for the sum over F frames (detrend=False, return_onesided=True)"""
    import torch
    if scaling not in ("density", "spectrum"):
        raise ValueError(f"scaling must be 'density' or 'spectrum', not {scaling!r}")
    w64 = torch.ones(n, dtype=torch.float64, device=device) if w is None else w.double()
    base = 1.0 / (F * float(fs) * float((w64 * w64).sum())) if scaling == "density" else 1.0 / (F * float(w64.sum()) ** 2)
    s = torch.full((n // 2 + 1,), 2.0 * base, dtype=torch.float64, device=device)
    s[0] = s[-1] = base
    return s


def _helper_args(n, hop, T, C, F):
    hop = n // 2 if hop is None else int(hop)          # scipy's default overlap
    if hop < 1:
        raise ValueError(f"hop must be at least 1, not {hop}")
    F = F(hop)
    T = default_T(C, F, n) if T is None else int(T)
    if T < 1:
        raise ValueError(f"T must be at least 1, not {T}")
    return hop, F, T


def welch(x, fs=1.0, window=None, n=512, hop=None, scaling="density", T=None):
    """the Welch estimate of the power spectral density ('density') or the power spectrum ('spectrum') of x: (streams, L) or (L,) ->
    (streams, n / 2 + 1) float32, the mean over ALL frames of n samples at hop (None: n / 2) of |X|^2 under scipy's scaling with
    detrend=False and return_onesided=True -- sum / (F fs sum w^2) or sum / (F (sum w)^2), times 2 on every bin but 0 and n / 2.  The
    frames are summed T at a time in the kernel (None: default_T) and the partial spectra in torch"""
    n = _check(n)
    s = _check_signal(x, "x", n)
    w = _check_window(window, n, s)
    _on_device(s, "welch")
    L = s.shape[-1]
    C = s.numel() // L
    hop, F, T = _helper_args(n, hop, T, C, lambda h: 1 + (L - n) // h)
    total = _all_frames(F, T, lambda first, G, t: _auto(s, w, n, C, L, first, G, t, hop, None))
    return (total.double() * _scale(n, F, w, fs, scaling, s.device)).float()


def csd(x, y, fs=1.0, window=None, n=512, hop=None, scaling="density", T=None):
    """the cross spectral density of x and y, mean over all frames of conj(X) Y under the scaling of welch(): (streams, n / 2 + 1)
    complex64 (scipy.signal.csd with detrend=False)"""
    n = _check(n)
    x, y, C, L, y_stride = _pair(x, y, n)
    w = _check_window(window, n, x)
    _on_device(x, "csd")
    hop, F, T = _helper_args(n, hop, T, C, lambda h: 1 + (L - n) // h)
    total = _all_frames(F, T, lambda first, G, t: _cross(x, y, w, n, C, L, y_stride, first, G, t, hop, None))
    import torch
    return (total.to(torch.complex128) * _scale(n, F, w, fs, scaling, x.device)).to(torch.complex64)


def coherence(x, y, window=None, n=512, hop=None, T=None):
    """the magnitude-squared coherence |Pxy|^2 / (Pxx Pyy) of x and y, (streams, n / 2 + 1) float32, from three launches over the same
    frames (two auto spectra and one cross spectrum; the scaling cancels).  Bins where Pxx Pyy is zero give NaN, as scipy's do"""
    n = _check(n)
    x, y, C, L, y_stride = _pair(x, y, n)
    w = _check_window(window, n, x)
    _on_device(x, "coherence")
    hop, F, T = _helper_args(n, hop, T, C, lambda h: 1 + (L - n) // h)
    pxx = _all_frames(F, T, lambda first, G, t: _auto(x, w, n, C, L, first, G, t, hop, None)).double()
    ys = y.reshape(-1, L)
    pyy = _all_frames(F, T, lambda first, G, t: _auto(ys, w, n, ys.shape[0], L, first, G, t, hop, None)).double()
    pxy = _all_frames(F, T, lambda first, G, t: _cross(x, y, w, n, C, L, y_stride, first, G, t, hop, None))
    import torch
    return (pxy.to(torch.complex128).abs() ** 2 / (pxx * pyy)).float()

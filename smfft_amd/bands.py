"""ctypes mirror of include/smfft_bands.h: band spectrograms of real signals (libsmfft_bands.so: the powers of the frames of
smfft_amd.stft -- n = 512 ... 8192 samples, powers of two, at any hop -- summed along frequency into the bands of a prepared table
inside the kernel: mel, Bark or octave bands, or plain re-binning; the frames' n / 2 + 1 powers never reach memory).  float32 in and out:

    band_spectrogram(s, plan, hop, w)[c, f, b] = sum_i weight[b][i] |stft(s, n, hop, w)[c, f, first[b] + i]|^2        one launch
    mel_spectrogram(s, fs, n, hop, n_mels, ...) = spectrogram(s, n, hop, w) @ mel_filterbank(n, fs, n_mels, ...).T
                                                  (torchaudio.transforms.MelSpectrogram(power=2) transposed), optionally ln or dB

A band table is three arrays: first[b] and count[b], the consecutive bins first[b] ... first[b] + count[b] - 1 of band b, and the
weights of all bands concatenated in band order (float32).  from_dense() cuts one out of a dense (bands, n / 2 + 1) matrix,
mel_filterbank() builds torchaudio's triangular filters as such a matrix, uniform_bands() re-bins; prepare() checks a table (every
rule of the header, on the host) and puts its plan on the device.  A dense matrix is a GEMM's job: a table holds at most
4 (n / 2 + 1) weights.

The library is loaded on first use, so that `import smfft_amd` behaves the same whether it was built or not.  The functions take
tensors on the device; the *_ptr and benchmark forms take device pointers as plain integers.  Timings are ADDED to a running total,
as in smfft_amd.api.  Refusals are raised before a device is touched.  There is no CPU fallback: a missing library raises on first
call.
"""
import ctypes

import numpy as np

from . import _addon
from ._rows import check_tensor as _check_tensor
from .stft import hann  # noqa: F401  (the periodic Hann window, for callers of this module)

SIZES = (256, 512, 1024, 2048, 4096)          # the inner transform lengths M = n / 2
LENGTHS = (512, 1024, 2048, 4096, 8192)       # the frame lengths n

_vp, _i, _ll, _dp = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.POINTER(ctypes.c_double)
_BANDS = [_vp, _vp, _vp, _vp, _i, _i, _i, _ll, _ll, _ll, _ll]    # d_in, d_out, d_window, d_plan, n, bands, weights, streams, frames, hop, stream_stride
_TABLE = [_i, _i, _vp, _vp, _vp]                                  # n, bands, h_first, h_count, h_weights
# name -> (restype, argtypes), exactly the declarations of include/smfft_bands.h (tests/test_sm_bands_cpu.py compares them)
SIGS = {
    "smfft_bands_fft_size": (_i, [_i]),
    "smfft_bands_frames": (_ll, [_ll, _i, _ll]),
    "smfft_bands_plan_bytes": (_ll, [_i, _i, _i]),
    "smfft_bands_tables": (_i, _TABLE + [_vp]),
    "smfft_bands_prepare": (_i, _TABLE + [_vp, _vp]),
    "smfft_bands_launch": (_i, _BANDS + [_vp]),
    "smfft_bands_launch_tuned": (_i, _BANDS + [_vp, _i]),
    "smfft_bands_benchmark": (_i, _BANDS + [_dp]),
}

LIB_PATH, load, lib = _addon.loader("libsmfft_bands.so", "SMFFT_BANDS_LIB", __name__, SIGS)
_lib = None


def _check(n):
    n = int(n)
    if n not in LENGTHS:
        raise ValueError(f"smfft_amd.bands serves n in {LENGTHS}, not {n}")
    return n


def _raise(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} -> {rc}")


def fft_size(n):
    """M = n / 2, the length of the kernels' complex transform (smfft_bands_fft_size)"""
    return lib().smfft_bands_fft_size(_check(n))


def frames(L, n, hop):
    """the whole frames of n samples at hop in L samples: 1 + (L - n) // hop, 0 for L < n (smfft_bands_frames)"""
    count = lib().smfft_bands_frames(int(L), _check(n), int(hop))
    if count < 0:
        raise ValueError(f"smfft_bands_frames(L={L}, n={n}, hop={hop}) -> {count}")
    return count


def plan_bytes(n, bands, weights):
    """12 bands + 4 weights, the bytes of a plan (smfft_bands_plan_bytes); ValueError for what the library refuses"""
    size = lib().smfft_bands_plan_bytes(int(n), int(bands), int(weights))
    if size < 0:
        raise ValueError(f"smfft_bands_plan_bytes(n={n}, bands={bands}, weights={weights}) -> {size}")
    return size


# ---- band tables (host) ----------------------------------------------------------------------------------------------------------------
def _table(first, count, weights):
    first, count = (np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.int64) for a in (first, count))
    weights = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1)).astype(np.float32)
    if first.shape != count.shape:
        raise ValueError(f"first and count must hold one entry per band, not {first.size} and {count.size}")
    if first.size and (np.abs(first).max() >= 2 ** 31 or np.abs(count).max() >= 2 ** 31):
        raise ValueError("first and count must fit int32")
    if count.size and (count.min() < 0 or int(count.sum()) != weights.size):
        raise ValueError(f"weights must hold sum(count) = {int(count.sum())} floats and every count be >= 0, not {weights.size}")
    return first.astype(np.int32), count.astype(np.int32), weights


def tables(n, first, count, weights):
    """the plan of a band table as host bytes (np.uint8 of plan_bytes: int32 first[], count[], offset[], then the float32 weights),
    after the library's check of every rule of the header (smfft_bands_tables: host only); ValueError for a table it refuses"""
    first, count, weights = _table(first, count, weights)
    size = lib().smfft_bands_plan_bytes(int(n), first.size, weights.size)
    if size < 0:
        raise ValueError(f"a band table of {first.size} bands and {weights.size} weights at n = {n} is refused: n in {LENGTHS}, "
                         f"1 <= bands <= n / 2 + 1, weights <= 4 (n / 2 + 1)")
    plan = np.zeros(size, np.uint8)
    rc = lib().smfft_bands_tables(int(n), first.size, first.ctypes.data, count.ctypes.data, weights.ctypes.data, plan.ctypes.data)
    if rc != 0:
        raise ValueError(f"smfft_bands_tables(n={n}, bands={first.size}) -> {rc}: a band reaches outside bins 0 ... n / 2")
    return plan


class Plan:
    """a prepared band table: `tensor`, the plan's bytes (torch.uint8) on a device, beside n, bands, weights (their number) and the
    host arrays first, count (int32) and w (float32, all bands' weights in band order)"""

    def __init__(self, tensor, n, first, count, w):
        self.tensor, self.n, self.first, self.count, self.w = tensor, n, first, count, w
        self.bands, self.weights = int(first.size), int(w.size)

    def dense(self, dtype=np.float64):
        """the table as a (bands, n / 2 + 1) matrix of the float32 weights taken exactly"""
        return to_dense(self.n, self.first, self.count, self.w, dtype)


def prepare(n, first, count, weights, device="cuda"):
    """a Plan of the band table on `device`: checked and laid out on the host by the library (tables()), then one copy"""
    import torch
    n = _check(n)
    first, count, w = _table(first, count, weights)
    host = tables(n, first, count, w)
    return Plan(torch.from_numpy(host).to(device), n, first, count, w)


def prepare_ptr(n, first, count, weights, d_plan, stream=0):
    """the same through smfft_bands_prepare: the plan is built on the host, copied to the plan_bytes bytes at d_plan on `stream` and
    waited for.  Returns the number of weights"""
    first, count, w = _table(first, count, weights)
    rc = lib().smfft_bands_prepare(int(n), first.size, first.ctypes.data, count.ctypes.data, w.ctypes.data, d_plan, stream)
    if rc == -1:
        raise ValueError(f"smfft_bands_prepare(n={n}, bands={first.size}) -> -1")
    _raise(rc, f"smfft_bands_prepare(n={n}, bands={first.size})")
    return int(w.size)


def from_dense(n, W):
    """the band table (first, count, weights) of a dense (bands, n / 2 + 1) matrix: the support of a row runs from its first to its
    last non-zero entry (zeros between them are kept as weights), a row of zeros is an empty band.  ValueError where the supports
    hold more than 4 (n / 2 + 1) weights or there are more than n / 2 + 1 rows: that is a dense matrix, a GEMM's job"""
    n = _check(n)
    W = np.asarray(W)
    bins = n // 2 + 1
    if W.ndim != 2 or W.shape[1] != bins or not 1 <= W.shape[0] <= bins:
        raise ValueError(f"W must be (bands, n / 2 + 1 = {bins}) with 1 <= bands <= {bins}, not {W.shape}")
    first, count, weights = np.zeros(W.shape[0], np.int32), np.zeros(W.shape[0], np.int32), []
    for b, row in enumerate(W):
        nz = np.flatnonzero(row)
        if nz.size:
            first[b], count[b] = nz[0], nz[-1] - nz[0] + 1
            weights.append(row[nz[0]:nz[-1] + 1])
    total = int(count.sum())
    if total > 4 * bins:
        raise ValueError(f"the rows' supports hold {total} weights, more than 4 (n / 2 + 1) = {4 * bins}: a dense matrix is a GEMM's job")
    return first, count, (np.concatenate(weights) if weights else np.zeros(0)).astype(np.float32)


def to_dense(n, first, count, weights, dtype=np.float64):
    """a band table expanded back: (bands, n / 2 + 1), overlapping nothing -- every band has a row of its own"""
    first, count, weights = _table(first, count, weights)
    W = np.zeros((first.size, _check(n) // 2 + 1), dtype)
    at = 0
    for b in range(first.size):
        W[b, first[b]:first[b] + count[b]] = weights[at:at + count[b]]
        at += count[b]
    return W


def _hz_to_mel(f, scale):
    f = np.asarray(f, np.float64)
    if scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    # Slaney's Auditory Toolbox: linear below 1 kHz (200 / 3 Hz per mel), logarithmic above (27 mels per factor 6.4)
    f_sp, min_log_hz, logstep = 200.0 / 3.0, 1000.0, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_hz / f_sp + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m, scale):
    m = np.asarray(m, np.float64)
    if scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    f_sp, min_log_hz, logstep = 200.0 / 3.0, 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filterbank(n, sample_rate, n_mels, f_min=0.0, f_max=None, mel_scale="htk", norm=None):
    """the triangular mel filters of torchaudio.functional.melscale_fbanks(n / 2 + 1, f_min, f_max, n_mels, sample_rate, norm,
    mel_scale), transposed: a dense (n_mels, n / 2 + 1) float64 matrix.  Bin k stands at k sample_rate / n Hz; n_mels + 2 points
    equally spaced in mel between f_min and f_max (None: sample_rate / 2) are the filters' feet and peaks f_0 ... f_{n_mels + 1}, and
    filter b is max(0, min((f - f_b) / (f_{b+1} - f_b), (f_{b+2} - f) / (f_{b+2} - f_{b+1}))).  mel_scale "htk": mel = 2595
    log10(1 + f / 700); "slaney": f / (200 / 3) below 1 kHz and 15 + 27 ln(f / 1000) / ln 6.4 above.  norm "slaney": filter b times
    2 / (f_{b+2} - f_b), unit area per filter"""
    n = _check(n)
    if mel_scale not in ("htk", "slaney"):
        raise ValueError(f"mel_scale must be 'htk' or 'slaney', not {mel_scale!r}")
    if norm not in (None, "slaney"):
        raise ValueError(f"norm must be None or 'slaney', not {norm!r}")
    n_mels = int(n_mels)
    f_max = sample_rate / 2.0 if f_max is None else float(f_max)
    if n_mels < 1 or not 0.0 <= f_min < f_max:
        raise ValueError(f"n_mels >= 1 and 0 <= f_min < f_max, not n_mels={n_mels}, f_min={f_min}, f_max={f_max}")
    freqs = np.linspace(0.0, sample_rate / 2.0, n // 2 + 1)
    pts = _mel_to_hz(np.linspace(_hz_to_mel(f_min, mel_scale), _hz_to_mel(f_max, mel_scale), n_mels + 2), mel_scale)
    diff = pts[1:] - pts[:-1]
    slopes = pts[None, :] - freqs[:, None]                      # (bins, n_mels + 2)
    down, up = -slopes[:, :-2] / diff[:-1], slopes[:, 2:] / diff[1:]
    fb = np.maximum(0.0, np.minimum(down, up))
    if norm == "slaney":
        fb = fb * (2.0 / (pts[2:] - pts[:-2]))[None, :]
    return np.ascontiguousarray(fb.T)


def uniform_bands(n, width):
    """re-binning: the band table (first, count, weights) of ceil((n / 2 + 1) / width) bands of `width` consecutive bins each (the
    last one shorter), all weights 1.0"""
    n, width = _check(n), int(width)
    bins = n // 2 + 1
    if not 1 <= width <= bins:
        raise ValueError(f"width must be in 1 ... n / 2 + 1 = {bins}, not {width}")
    first = np.arange(0, bins, width, dtype=np.int32)
    count = np.minimum(width, bins - first).astype(np.int32)
    return first, count, np.ones(int(count.sum()), np.float32)


# ---- device pointers -------------------------------------------------------------------------------------------------------------------
def launch_ptr(d_in, d_out, d_window, d_plan, n, bands, weights, streams, frames, hop, stream_stride, stream=0, grid=None):
    """streams * frames rows of `bands` float32: frame (c, f) reads d_in[c stream_stride + f hop ... + n) and writes its band sums at
    element (c frames + f) bands of d_out; d_window: n floats or None; d_plan: the plan of a table of `bands` bands and `weights`
    weights (smfft_bands_launch; grid: on that many workgroups, smfft_bands_launch_tuned)"""
    if grid is None:
        rc = lib().smfft_bands_launch(d_in, d_out, d_window, d_plan, n, bands, weights, streams, frames, hop, stream_stride, stream)
    else:
        rc = lib().smfft_bands_launch_tuned(d_in, d_out, d_window, d_plan, n, bands, weights, streams, frames, hop, stream_stride, stream, grid)
    _raise(rc, f"smfft_bands_launch(n={n}, bands={bands}, weights={weights}, streams={streams}, frames={frames}, hop={hop}, stream_stride={stream_stride}, grid={grid})")


def benchmark(d_in, d_out, d_window, d_plan, n, bands, weights, streams, frames, hop, stream_stride):
    """One launch on the null stream, timed with events; synchronous.  Returns (status, elapsed_ms)."""
    t = ctypes.c_double(0.0)
    rc = lib().smfft_bands_benchmark(d_in, d_out, d_window, d_plan, n, bands, weights, streams, frames, hop, stream_stride, ctypes.byref(t))
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


def _check_plan(plan, x):
    if not isinstance(plan, Plan):
        raise TypeError(f"plan must be a smfft_amd.bands.Plan (prepare()), not {type(plan).__name__}")
    if plan.tensor.device != x.device:
        raise ValueError(f"the plan must be on the signal's device: {plan.tensor.device} against {x.device}")
    return plan


def _on_device(x, what):
    if not x.is_cuda:
        raise ValueError(f"smfft_amd.bands.{what} takes tensors on the device.  There is no CPU fallback")


def _stream(x, stream):
    import torch
    return torch.cuda.current_stream(x.device).cuda_stream if stream is None else stream


def launch(signal, out, plan, hop, window=None, stream=None):
    """signal: (streams, L) or (L,) contiguous float32 on the device, L >= plan.n -> out: (streams, frames, plan.bands) float32,
    frames = 1 + (L - n) // hop, in one launch that reads every sample from the signal itself.  out None: a new tensor; else a
    contiguous float32 tensor of that shape on the signal's device, which is returned.  Enqueues on `stream` (a hipStream_t as an
    integer; None = torch's current stream of the signal's device); nothing is synchronised"""
    s = _check_tensor(signal, "signal")
    if not isinstance(plan, Plan):
        raise TypeError(f"plan must be a smfft_amd.bands.Plan (prepare()), not {type(plan).__name__}")
    n, hop = plan.n, int(hop)
    if s.ndim > 2 or s.shape[-1] < n:
        raise ValueError(f"signal must be (streams, L) or (L,) with L >= n = {n}, not {tuple(s.shape)}")
    if hop < 1:
        raise ValueError(f"hop must be at least 1, not {hop}")
    w = _check_window(window, n, s)
    L = s.shape[-1]
    C = s.numel() // L
    F = 1 + (L - n) // hop
    if out is not None:
        out = _check_tensor(out, "out")
        if out.shape != (C, F, plan.bands) or out.device != s.device:
            raise ValueError(f"out must be {(C, F, plan.bands)} on the signal's device, not {tuple(out.shape)} on {out.device}")
    _on_device(s, "launch")
    _check_plan(plan, s)
    import torch
    handle = lib()
    if out is None:
        out = torch.empty((C, F, plan.bands), dtype=torch.float32, device=s.device)
    with torch.cuda.device(s.device):
        rc = handle.smfft_bands_launch(s.data_ptr(), out.data_ptr(), None if w is None else w.data_ptr(), plan.tensor.data_ptr(), n, plan.bands,
                                       plan.weights, C, F, hop, L, _stream(s, stream))
    _raise(rc, f"smfft_bands_launch(n={n}, bands={plan.bands}, weights={plan.weights}, streams={C}, frames={F}, hop={hop}, stream_stride={L})")
    return out


def _centered(signal, n):
    """reflect-pads n / 2 samples on each side, in plain torch (one padded copy of the signal): torch.stft(center=True)'s frames"""
    s = _check_tensor(signal, "signal")
    if s.ndim > 2 or s.shape[-1] <= n // 2:
        raise ValueError(f"signal must be (streams, L) or (L,) with L > n / 2 = {n // 2} for reflect padding, not {tuple(s.shape)}")
    import torch
    return torch.nn.functional.pad(s.reshape(-1, s.shape[-1]).unsqueeze(0), (n // 2, n // 2), mode="reflect").squeeze(0).contiguous()


def band_spectrogram(signal, plan, hop, window=None, center=False):
    """(streams, frames, plan.bands) float32: the band sums of the power spectrogram of signal (streams, L) or (L,), one launch.
    window: n float32 on the same device, or None for all ones.  center=True reflect-pads n / 2 samples on each side first, as
    smfft_amd.stft.stft does"""
    if not isinstance(plan, Plan):
        raise TypeError(f"plan must be a smfft_amd.bands.Plan (prepare()), not {type(plan).__name__}")
    if center:
        signal = _centered(signal, plan.n)
    return launch(signal, None, plan, hop, window)


_MEL_PLANS = {}       # (the arguments of mel_filterbank, device type, device index) -> Plan; at most _MEL_PLANS_KEPT, the oldest leaves first
_MEL_PLANS_KEPT = 8


def _mel_key(n, sample_rate, n_mels, f_min, f_max, mel_scale, norm):
    return (_check(n), float(sample_rate), int(n_mels), float(f_min), None if f_max is None else float(f_max), mel_scale, norm)


def mel_plan(n, sample_rate, n_mels, f_min=0.0, f_max=None, mel_scale="htk", norm=None, device="cuda"):
    """the Plan of mel_filterbank(...) on `device`.  The last 8 plans made here are kept for the life of the process (a few tens of
    kilobytes of device memory each), keyed by the arguments and the resolved device -- "cuda" is the current device, the same entry
    as its "cuda:<index>" -- so that mel_spectrogram prepares a table once; a ninth drops the oldest"""
    import torch
    dev = torch.device(device)
    index = dev.index if dev.index is not None or dev.type != "cuda" else torch.cuda.current_device()
    key = _mel_key(n, sample_rate, n_mels, f_min, f_max, mel_scale, norm) + (dev.type, index)
    plan = _MEL_PLANS.pop(key, None)
    if plan is None:
        plan = prepare(n, *from_dense(n, mel_filterbank(n, sample_rate, n_mels, f_min, f_max, mel_scale, norm)), device=torch.device(dev.type, index))
    _MEL_PLANS[key] = plan                     # (again) the youngest
    while len(_MEL_PLANS) > _MEL_PLANS_KEPT:
        del _MEL_PLANS[next(iter(_MEL_PLANS))]
    return plan


def mel_spectrogram(signal, sample_rate, n, hop, n_mels, f_min=0.0, f_max=None, mel_scale="htk", norm=None, window=None, center=False,
                    log=None, floor=1e-10):
    """(streams, frames, n_mels) float32: the mel spectrogram of signal under mel_filterbank(n, sample_rate, n_mels, f_min, f_max,
    mel_scale, norm), one launch.  log None: the band powers; "ln": ln(max(., floor)); "db": 10 log10(max(., floor)) -- plain torch
    on the small output"""
    if log not in (None, "ln", "db"):
        raise ValueError(f"log must be None, 'ln' or 'db', not {log!r}")
    n = _check(n)
    s = _check_tensor(signal, "signal")
    _check_window(window, n, s)
    # the filter bank's own refusals, before a device is touched
    if mel_scale not in ("htk", "slaney") or norm not in (None, "slaney") or int(n_mels) < 1 or not 0.0 <= f_min < (sample_rate / 2.0 if f_max is None else f_max):
        mel_filterbank(n, sample_rate, n_mels, f_min, f_max, mel_scale, norm)
    _on_device(s, "mel_spectrogram")
    out = band_spectrogram(s, mel_plan(n, sample_rate, n_mels, f_min, f_max, mel_scale, norm, s.device), hop, window, center)
    if log is None:
        return out
    import torch
    out = torch.log(out.clamp_(min=floor)) if log == "ln" else torch.log10(out.clamp_(min=floor)).mul_(10.0)
    return out

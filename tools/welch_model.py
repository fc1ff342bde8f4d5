"""NumPy model of libsmfft_welch.so (smfft_amd/csrc/smfft_welch.hip): the frames of tools/stft_model.py summed over T consecutive frames
per group, as powers (auto spectra) or as conj(X) Y (cross spectra), and scipy's scaling of such sums.  The frame-to-spectrum step is
stft_model.chain; nothing of it is written again here.

    auto(fr, T, w, dtype)            fr: (..., F, n) frames -> (..., F // T, M + 1): sum_t |X|^2 per group of T frames.  dtype=np.float64:
                                     the fp64 reference of the GPU tests; np.float32: stft_model's fp32 chain per frame and the kernel's
                                     sequential fp32 sum in frame order (acc = p_0, acc += p_t)
    cross(fx, fy, T, w, dtype)       the same for sum_t conj(X) Y, complex; float32: re = xr yr + xi yi and im = xr yi - xi yr, every
                                     product and sum rounded (the kernel fuses one product of re: a floor, not a bound), summed per
                                     component in frame order
    direct_auto / direct_cross       the same sums from the O(n^2) sums of the definition (stft_model.direct), fp64
    sequential_sum(p, T)             (..., F, K) float32 -> (..., F // T, K): the fp32 sum in frame order of values as they are
    scale(n, F, w, fs, scaling)      (M + 1,) factors that turn the sum over all F frames into scipy.signal.welch / csd with
                                     detrend=False, return_onesided=True: 1 / (F fs sum w^2) ('density') or 1 / (F (sum w)^2)
                                     ('spectrum'), times 2 on every bin but 0 and M
    coherence(pxx, pyy, pxy)         |Pxy|^2 / (Pxx Pyy)
    errors(got, want, norm)          per spectrum: ||d||_2 / ||norm||_2 and max |d| / max |norm| (norm: want, or the sqrt(Pxx Pyy) that
                                     bounds a cross spectrum)
"""
import numpy as np

import stft_model as sm


def _groups(a, T):
    """(..., F, K) -> (..., F // T, T, K): the whole groups of T frames"""
    F = a.shape[-2]
    G = F // T
    return a[..., :G * T, :].reshape(a.shape[:-2] + (G, T, a.shape[-1]))


def sequential_sum(p, T):
    """the kernel's sum: per group acc = p_0, then acc += p_t in frame order, in the dtype of p (complex: per component)"""
    g = _groups(np.asarray(p), T)
    acc = g[..., 0, :].copy()
    for t in range(1, T):
        acc = (acc + g[..., t, :]).astype(p.dtype)
    return acc


def auto(fr, T, w=None, dtype=np.float64):
    p = sm.chain(fr, w, dtype, power=True)
    if dtype == np.float64:
        return _groups(p, T).sum(axis=-2)
    return sequential_sum(p, T)


def cross(fx, fy, T, w=None, dtype=np.float64):
    X, Y = sm.chain(fx, w, dtype), sm.chain(fy, w, dtype)
    if dtype == np.float64:
        return _groups(np.conj(X) * Y, T).sum(axis=-2)
    xr, xi, yr, yi = X.real, X.imag, Y.real, Y.imag
    re = ((xr * yr).astype(dtype) + (xi * yi).astype(dtype)).astype(dtype)
    im = ((xr * yi).astype(dtype) - (xi * yr).astype(dtype)).astype(dtype)
    return sequential_sum(re, T) + 1j * sequential_sum(im, T).astype(np.complex64)


def direct_auto(fr, T, w=None):
    return _groups(np.abs(sm.direct(fr, w)) ** 2, T).sum(axis=-2)


def direct_cross(fx, fy, T, w=None):
    return _groups(np.conj(sm.direct(fx, w)) * sm.direct(fy, w), T).sum(axis=-2)


def scale(n, F, w=None, fs=1.0, scaling="density"):
    w = np.ones(n) if w is None else np.asarray(w, np.float64)
    if scaling == "density":
        base = 1.0 / (F * fs * np.sum(w * w))
    elif scaling == "spectrum":
        base = 1.0 / (F * np.sum(w) ** 2)
    else:
        raise ValueError(f"scaling must be 'density' or 'spectrum', not {scaling!r}")
    s = np.full(n // 2 + 1, 2.0 * base)
    s[0] = s[-1] = base
    return s


def coherence(pxx, pyy, pxy):
    return np.abs(pxy) ** 2 / (pxx * pyy)


def errors(got, want, norm=None):
    """(per-spectrum ||d||_2 / ||norm||_2, per-spectrum max |d| / max |norm|), spectra on the last axis; norm: want when not given"""
    got, want = np.asarray(got), np.asarray(want)
    norm = want if norm is None else np.asarray(norm)
    wide = np.complex128 if np.iscomplexobj(got) or np.iscomplexobj(want) else np.float64
    d = (got.astype(wide) - want.astype(wide)).reshape(-1, want.shape[-1])
    norm = np.abs(norm).reshape(-1, want.shape[-1])
    l2 = np.linalg.norm(d, axis=1) / np.maximum(np.linalg.norm(norm, axis=1), 1e-300)
    mx = np.max(np.abs(d), axis=1) / np.maximum(np.max(norm, axis=1), 1e-300)
    return l2, mx

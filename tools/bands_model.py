"""NumPy model of libsmfft_bands.so (smfft_amd/csrc/smfft_bands.hip): the powers of the frames of tools/stft_model.py summed along
frequency into the bands of a table.  The frame-to-spectrum step is stft_model.chain; nothing of it is written again here.

    dense(n, first, count, weights)          the table as a (bands, M + 1) float64 matrix of the float32 weights taken exactly
    bands(fr, first, count, weights, w, dtype)
                                             fr: (..., n) frames -> (..., bands).  dtype=np.float64: the fp64 reference of the GPU tests,
                                             dense(...) @ the fp64 chain's powers; np.float32, the staged mode: stft_model's fp32 chain
                                             per frame, then the kernel's stage -- every product w * p rounded to fp32 on its own and the
                                             sum sequential in fp32 in ascending bin order from -0; an empty band gives +0
    sequential(p, first, count, weights)     that stage alone on powers (..., M + 1) float32 as they are
    bounds(W, P, longest, row_l2, row_max)   per frame: kappa_2, kappa_inf and the two bounds of the GPU tests
    errors(got, ref, A)                      per frame: ||got - ref||_2 / ||A||_2 and max |got - ref| / max A
"""
import numpy as np

import stft_model as sm


def _table(first, count, weights):
    first, count = np.asarray(first, np.int64).reshape(-1), np.asarray(count, np.int64).reshape(-1)
    weights = np.asarray(weights, np.float32).reshape(-1)
    assert first.shape == count.shape and count.min() >= 0 and count.sum() == weights.size
    return first, count, weights, np.concatenate([[0], np.cumsum(count)])


def dense(n, first, count, weights):
    first, count, weights, offset = _table(first, count, weights)
    W = np.zeros((first.size, sm.check_n(n) // 2 + 1), np.float64)
    for b in range(first.size):
        assert 0 <= first[b] and first[b] + count[b] <= W.shape[1]
        W[b, first[b]:first[b] + count[b]] = weights[offset[b]:offset[b + 1]]
    return W


def sequential(p, first, count, weights):
    """(..., M + 1) float32 -> (..., bands) float32, the kernel's stage: per band acc = -0, then t = w_i * p_i and acc = acc + t in
    ascending bin order, every step rounded to fp32; an empty band gives +0"""
    p = np.asarray(p)
    assert p.dtype == np.float32
    first, count, weights, offset = _table(first, count, weights)
    out = np.zeros(p.shape[:-1] + (first.size,), np.float32)
    for b in range(first.size):
        if count[b] == 0:
            continue                                        # exactly +0
        acc = np.full(p.shape[:-1], -0.0, np.float32)
        for i in range(count[b]):
            t = (weights[offset[b] + i] * p[..., first[b] + i]).astype(np.float32)
            acc = (acc + t).astype(np.float32)
        out[..., b] = acc
    return out


def bands(fr, first, count, weights, w=None, dtype=np.float64):
    fr = np.asarray(fr)
    p = sm.chain(fr, w, dtype, power=True)
    if dtype == np.float64:
        return p @ dense(fr.shape[-1], first, count, weights).T
    return sequential(p, first, count, weights)


def bounds(W, P, longest, row_l2, row_max):
    """W: (bands, M + 1) fp64, P: (frames, M + 1) the fp64 chain's powers.  Per frame, with A = |W| P:
    kappa_2 = ||W||_2 ||P||_2 / ||A||_2 and kappa_inf = max_b sum_k |w_bk| max P / max A, and the bounds
    kappa_2 2 row_l2 + (longest + 1) 2^-24 and kappa_inf 2 row_max + (longest + 1) 2^-24.  Returns (k2, kinf, l2 bound, max bound)"""
    P = np.asarray(P, np.float64).reshape(-1, W.shape[1])
    A = P @ np.abs(W).T
    k2 = np.linalg.norm(W, 2) * np.linalg.norm(P, axis=1) / np.maximum(np.linalg.norm(A, axis=1), 1e-300)
    kinf = np.abs(W).sum(axis=1).max() * P.max(axis=1) / np.maximum(A.max(axis=1), 1e-300)
    tail = (longest + 1) * 2.0 ** -24
    return k2, kinf, k2 * 2 * row_l2 + tail, kinf * 2 * row_max + tail


def errors(got, ref, A):
    """(per-frame ||got - ref||_2 / ||A||_2, per-frame max |got - ref| / max A), bands on the last axis"""
    ref = np.asarray(ref, np.float64)
    d = (np.asarray(got).astype(np.float64) - ref).reshape(-1, ref.shape[-1])
    A = np.abs(np.asarray(A, np.float64)).reshape(-1, ref.shape[-1])
    l2 = np.linalg.norm(d, axis=1) / np.maximum(np.linalg.norm(A, axis=1), 1e-300)
    mx = np.max(np.abs(d), axis=1) / np.maximum(np.max(A, axis=1), 1e-300)
    return l2, mx

"""NumPy model of the chain of libsmfft_dct.so (smfft_amd/csrc/smfft_dct.hip): DCT-II / DCT-III / DST-II / DST-III of rows of n points
through ONE complex transform of M = n / 2 points per row, un-normalised (scipy.fft's norm=None).

    direct(x, type, sine)            the sums of the definition in fp64, O(n^2) per row: the reference of the reference
    chain(x, type, sine, dtype)      the kernel's steps; dtype=np.float64: the fp64 reference of the GPU tests; np.float32: every stage
                                     rounded to fp32, the transform itself in fp64 and rounded once (so the model is a floor, not a bound)
    chain(..., fast_w4=True)         W_4n^k from fp32 sinf-grade values (the angle rounded to fp32 first) instead of fp64 rounded once

Forward (type II), v the permuted row (v[j] = x[2j], v[n-1-j] = x[2j+1]), z[p] = v[2p] + i v[2p+1], Z = DFT_M(z), P[k] = conj Z[(M-k) % M],
S = Z + P, D = Z - P, V = S - i W_n^k D (twice the n-point spectrum of v), Y = W_4n^k V, X[k] = Re Y[k] (k <= M), X[n-k] = -Im Y[k].
Inverse (type III) undoes it step by step; DST goes through the same chain with a sign on the odd samples and the other side reversed.
"""
import numpy as np

SIZES = (512, 1024, 2048, 4096, 8192)


def check_n(n):
    if n not in SIZES:
        raise ValueError(f"n must be one of {SIZES}, not {n}")
    return n


def direct(x, type=2, sine=False):
    """the definition, fp64: rows on the last axis"""
    x = np.asarray(x, np.float64)
    n = x.shape[-1]
    j = np.arange(n)
    if type == 2:
        k = np.arange(1, n + 1) if sine else np.arange(n)
        f = np.sin if sine else np.cos
        return 2.0 * x @ f(np.pi * np.outer(2 * j + 1, k) / (2 * n))
    if type != 3:
        raise ValueError("type must be 2 or 3")
    if sine:
        k = np.arange(1, n)
        return np.where(j % 2 == 0, 1.0, -1.0) * x[..., n - 1:n] + 2.0 * x[..., :n - 1] @ np.sin(np.pi * np.outer(k, 2 * j + 1) / (2 * n))
    k = np.arange(1, n)
    return x[..., :1] + 2.0 * x[..., 1:] @ np.cos(np.pi * np.outer(k, 2 * j + 1) / (2 * n))


def pack_index(n):
    """(i0, i1): z[p] = row[i0[p]] + i row[i1[p]], p < M = n / 2; the second half (p >= M / 2) holds the odd samples"""
    M = n // 2
    p = np.arange(M)
    lo = p < M // 2
    return np.where(lo, 4 * p, 2 * n - 1 - 4 * p), np.where(lo, 4 * p + 2, 2 * n - 3 - 4 * p)


def twiddles(n, dtype, fast_w4=False):
    """(W_n^k, k < M; W_4n^k, k <= M) as complex arrays of the precision of dtype: fp64 values rounded once"""
    M = n // 2
    ctype = np.complex64 if dtype == np.float32 else np.complex128
    wn = np.exp(-2j * np.pi * np.arange(M) / n).astype(ctype)
    if fast_w4:
        ang = (np.float32(2 * np.pi) * np.arange(M + 1, dtype=np.float32) / np.float32(4 * n)).astype(np.float32)
        w4 = (np.cos(ang.astype(np.float64)) - 1j * np.sin(ang.astype(np.float64))).astype(ctype)
    else:
        w4 = np.exp(-2j * np.pi * np.arange(M + 1) / (4 * n)).astype(ctype)
    return wn, w4


def chain(x, type=2, sine=False, dtype=np.float64, fast_w4=False):
    x = np.asarray(x)
    n = check_n(x.shape[-1])
    M = n // 2
    ctype = np.complex64 if dtype == np.float32 else np.complex128
    i0, i1 = pack_index(n)
    sign = np.where((np.arange(M) >= M // 2) & bool(sine), -1.0, 1.0).astype(dtype)
    wn, w4 = twiddles(n, dtype, fast_w4)
    x = x.astype(dtype)
    if type == 2:
        z = ((x[..., i0] + 1j * x[..., i1]) * sign).astype(ctype)
        Z = np.fft.fft(z.astype(np.complex128), axis=-1).astype(ctype)
        P = np.conj(Z[..., (M - np.arange(M)) % M])
        S, D = (Z + P).astype(ctype), (Z - P).astype(ctype)
        V = (S - 1j * (wn * D).astype(ctype)).astype(ctype)
        Y = (w4[:M] * V).astype(ctype)
        X = np.empty(x.shape, dtype)
        X[..., :M] = Y.real
        X[..., M + 1:] = -Y.imag[..., :0:-1]                        # X[n - k], k = M - 1 ... 1
        X[..., M] = (2 * (w4[M].real * (Z[..., 0].real - Z[..., 0].imag).astype(dtype))).astype(dtype)
        return X[..., ::-1] if sine else X
    if type != 3:
        raise ValueError("type must be 2 or 3")
    X = x[..., ::-1] if sine else x
    Xn = np.concatenate([X, np.zeros(X.shape[:-1] + (1,), dtype)], axis=-1)       # X[n] := 0
    k = np.arange(M)
    Vk = (np.conj(w4[k]) * (Xn[..., k] - 1j * Xn[..., n - k])).astype(ctype)
    Vm = (np.conj(w4[M - k]) * (Xn[..., M - k] - 1j * Xn[..., M + k])).astype(ctype)
    A, B = (Vk + np.conj(Vm)).astype(ctype), (Vk - np.conj(Vm)).astype(ctype)
    Z = (A + 1j * (np.conj(wn) * B).astype(ctype)).astype(ctype)
    z = (np.fft.ifft(Z.astype(np.complex128), axis=-1) * M).astype(ctype)
    y = np.empty(x.shape, dtype)
    y[..., i0] = z.real * sign
    y[..., i1] = z.imag * sign
    return y


def errors(got, want):
    """(worst row relL2, worst row max |d| / max |want|) of rows on the last axis"""
    got, want = np.asarray(got, np.float64).reshape(-1, got.shape[-1]), np.asarray(want, np.float64).reshape(-1, want.shape[-1])
    d = got - want
    l2 = np.linalg.norm(d, axis=1) / np.maximum(np.linalg.norm(want, axis=1), 1e-300)
    mx = np.max(np.abs(d), axis=1) / np.maximum(np.max(np.abs(want), axis=1), 1e-300)
    return float(l2.max()), float(mx.max())

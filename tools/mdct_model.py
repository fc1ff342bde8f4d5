"""NumPy model of the chain of libsmfft_mdct.so (smfft_amd/csrc/smfft_mdct.hip): DCT-IV / DST-IV of rows of n points and the MDCT / IMDCT
of N coefficients per frame of 2 N samples, through ONE complex transform of M = n / 2 (N / 2) points per row, un-normalised (scipy.fft's
norm=None for the type IV transforms).

    direct(x, sine)                  the DCT-IV / DST-IV sums of the definition in fp64, O(n^2) per row: the reference of the reference
    mdct_direct(x, w), imdct_direct(X, w)   the MDCT / IMDCT sums of the definition in fp64
    chain(x, sine, dtype)            the kernel's steps; dtype=np.float64: the fp64 reference of the GPU tests; np.float32: every stage
                                     rounded to fp32, the transform itself in fp64 and rounded once (so the model is a floor, not a bound)
    mdct_chain(x, w, dtype), imdct_chain(X, w, dtype)   the same for the lapped transforms (w=None: all ones)
    fold_index(N), unfold_index(N)   the index rows of the fold in front of the MDCT and of the unfold behind the IMDCT
    frames(s, N), overlap_add(y)     the frames of 2 N samples at hop N of a signal, and the sum that undoes them

Type IV, with M = n / 2 and p, k < M:
    t[p] = (x[2p] + i x[n-1-2p]) exp(-i pi (4p+1) / (4n));  T = DFT_M(t);  Y[k] = T[k] exp(-i pi k / n);
    X[2k] = 2 Re Y[k];  X[n-1-2k] = -2 Im Y[k].
Why: with c = (2k'+1)(2j+1) pi / (4n), the sum over the even j = 2p at the even k' = 2k and the sum over the odd j = n-1-2p there are
the real part of one complex sum, and the odd k' = n-1-2k gives its imaginary part, because cos turns into -+sin under the two
reflections.  DST-IV(x)[k] = (-1)^k DCT-IV(reverse x)[k]: the row reversed on the load side, the sign on the store side.
MDCT(x) = DCT-IV_N(u) / 2 with u = [-c_r - d, a - b_r] the fold of v = w x = [a, b, c, d] (quarters of N / 2, _r reversed);
IMDCT(X) = w [D[N/2:], -reverse(D), -D[:N/2]] with D = DCT-IV_N(X) / 2.
"""
import numpy as np

SIZES = (512, 1024, 2048, 4096, 8192)


def check_n(n):
    if n not in SIZES:
        raise ValueError(f"n must be one of {SIZES}, not {n}")
    return n


def direct(x, sine=False):
    """the type IV definition, fp64: rows on the last axis"""
    x = np.asarray(x, np.float64)
    n = x.shape[-1]
    j = np.arange(n)
    f = np.sin if sine else np.cos
    return 2.0 * x @ f(np.pi * np.outer(2 * j + 1, 2 * j + 1) / (4 * n))


def _mdct_matrix(N):
    """cos(pi / N (j + 1/2 + N/2)(k + 1/2)), (2N, N)"""
    j, k = np.arange(2 * N), np.arange(N)
    return np.cos(np.pi / N * np.outer(j + 0.5 + N / 2, k + 0.5))


def _window(w, N, dtype=np.float64):
    return np.ones(2 * N, dtype) if w is None else np.asarray(w).astype(dtype)


def mdct_direct(x, w=None):
    x = np.asarray(x, np.float64)
    N = x.shape[-1] // 2
    return (x * _window(w, N)) @ _mdct_matrix(N)


def imdct_direct(X, w=None):
    X = np.asarray(X, np.float64)
    N = X.shape[-1]
    return (X @ _mdct_matrix(N).T) * _window(w, N)


def twiddles(n, dtype):
    """(exp(-i pi (4p+1) / (4n)), exp(-i pi k / n)), p, k < M, of the precision of dtype: fp64 values rounded once"""
    M = n // 2
    ctype = np.complex64 if dtype == np.float32 else np.complex128
    p = np.arange(M)
    return np.exp(-1j * np.pi * (4 * p + 1) / (4 * n)).astype(ctype), np.exp(-1j * np.pi * p / n).astype(ctype)


def _core(re, im, n, dtype, scale):
    """scale Re / -Im of the twiddled transform of re + i im, interleaved: out[2k] = scale Re Y[k], out[n-1-2k] = -scale Im Y[k]"""
    M = n // 2
    ctype = np.complex64 if dtype == np.float32 else np.complex128
    pre, post = twiddles(n, dtype)
    t = ((re + 1j * im).astype(ctype) * pre).astype(ctype)
    T = np.fft.fft(t.astype(np.complex128), axis=-1).astype(ctype)
    Y = (T * post).astype(ctype)
    X = np.empty(re.shape[:-1] + (n,), dtype)
    k = np.arange(M)
    X[..., 2 * k] = scale * Y.real
    X[..., n - 1 - 2 * k] = -scale * Y.imag
    return X


def chain(x, sine=False, dtype=np.float64):
    """DCT-IV (sine False) or DST-IV of rows on the last axis"""
    x = np.asarray(x)
    n = check_n(x.shape[-1])
    p = np.arange(n // 2)
    x = x.astype(dtype)
    if sine:
        x = x[..., ::-1]
    X = _core(x[..., 2 * p], x[..., n - 1 - 2 * p], n, dtype, 2.0)
    return X * np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(dtype) if sine else X


def fold_index(N):
    """(i0, s0, i1, s1): u[j] = s0[j] v[i0[j]] + s1[j] v[i1[j]], j < N, the fold u = [-c_r - d, a - b_r] of v = [a, b, c, d]"""
    h = N // 2
    j = np.arange(N)
    lo = j < h
    i0 = np.where(lo, N + h - 1 - j, j - h)          # c reversed | a
    i1 = np.where(lo, N + h + j, N + h - 1 - j)      # d | b reversed
    s0 = np.where(lo, -1.0, 1.0)
    s1 = np.full(N, -1.0)
    return i0, s0, i1, s1


def unfold_index(N):
    """(i, s): y[j] = w[j] s[j] D[i[j]], j < 2N, the unfold [D[N/2:], -reverse(D), -D[:N/2]]"""
    h = N // 2
    j = np.arange(2 * N)
    i = np.where(j < h, h + j, np.where(j < h + N, N + h - 1 - j, j - N - h))
    s = np.where(j < h, 1.0, -1.0)
    return i, s


def mdct_chain(x, w=None, dtype=np.float64):
    """MDCT of rows of 2 N samples on the last axis -> N coefficients"""
    x = np.asarray(x)
    N = check_n(x.shape[-1] // 2)
    if x.shape[-1] != 2 * N:
        raise ValueError("rows of 2 N samples")
    v = (x.astype(dtype) * _window(w, N, dtype)).astype(dtype)
    i0, s0, i1, s1 = fold_index(N)
    u = (s0.astype(dtype) * v[..., i0] + s1.astype(dtype) * v[..., i1]).astype(dtype)
    p = np.arange(N // 2)
    return _core(u[..., 2 * p], u[..., N - 1 - 2 * p], N, dtype, 1.0)


def imdct_chain(X, w=None, dtype=np.float64):
    """IMDCT of rows of N coefficients on the last axis -> 2 N samples"""
    X = np.asarray(X)
    N = check_n(X.shape[-1])
    p = np.arange(N // 2)
    X = X.astype(dtype)
    D = _core(X[..., 2 * p], X[..., N - 1 - 2 * p], N, dtype, 1.0)
    i, s = unfold_index(N)
    return ((s.astype(dtype) * D[..., i]) * _window(w, N, dtype)).astype(dtype)


def sine_window(N, dtype=np.float64):
    """sin(pi (j + 1/2) / (2N)), j < 2N: w[j]^2 + w[j+N]^2 = 1"""
    return np.sin(np.pi * (np.arange(2 * N) + 0.5) / (2 * N)).astype(dtype)


def frames(s, N):
    """(..., L) -> (..., L / N - 1, 2N): the frames of 2 N samples at hop N"""
    s = np.asarray(s)
    F = s.shape[-1] // N - 1
    return np.stack([s[..., f * N:f * N + 2 * N] for f in range(F)], axis=-2)


def overlap_add(y):
    """(..., F, 2N) -> (..., (F + 1) N): frame f added at offset f N"""
    y = np.asarray(y)
    F, N = y.shape[-2], y.shape[-1] // 2
    out = np.zeros(y.shape[:-2] + ((F + 1) * N,), y.dtype)
    for f in range(F):
        out[..., f * N:f * N + 2 * N] += y[..., f, :]
    return out


def errors(got, want):
    """(worst row relL2, worst row max |d| / max |want|) of rows on the last axis"""
    got, want = np.asarray(got, np.float64).reshape(-1, got.shape[-1]), np.asarray(want, np.float64).reshape(-1, want.shape[-1])
    d = got - want
    l2 = np.linalg.norm(d, axis=1) / np.maximum(np.linalg.norm(want, axis=1), 1e-300)
    mx = np.max(np.abs(d), axis=1) / np.maximum(np.max(np.abs(want), axis=1), 1e-300)
    return float(l2.max()), float(mx.max())

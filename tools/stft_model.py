"""NumPy model of the chain of libsmfft_stft.so (smfft_amd/csrc/smfft_stft.hip): the short-time Fourier transform of real frames of n
samples through ONE complex transform of M = n / 2 points per frame, and its inverse.

    direct(x, w)                     the sums of the definition in fp64, O(n^2) per frame: the reference of the reference
    chain(x, w, dtype, power)        the forward kernel's steps; dtype=np.float64: the fp64 reference of the GPU tests; np.float32:
                                     every stage rounded to fp32, the transform itself in fp64 and rounded once (so the model is a
                                     floor, not a bound)
    inverse_chain(X, w, dtype)       the same for the inverse kernel (w=None: all ones)
    frames(s, n, hop)                the frames of n samples at hop of a signal, copied out
    overlap_add(y, hop, w, length)   the sum of frames at hop, divided by the summed squared window where one is given
    hann(n)                          the periodic Hann window
    errors(got, want)                worst row relL2 and max |d| / max |want|

Forward, with p, k < M and W_n = exp(-2 pi i / n):
    z[p] = w[2p] x[2p] + i w[2p+1] x[2p+1];  Z = DFT_M(z);  P[k] = conj Z[(M-k) mod M];
    X[k] = (Z[k] + P[k]) / 2 - (i/2) W_n^k (Z[k] - P[k]);  X[0] = Re Z[0] + Im Z[0];  X[M] = Re Z[0] - Im Z[0].
Why: (Z + P) / 2 and (Z - P) / (2i) are the spectra of the even and of the odd samples, and X[k] = E[k] + W_n^k O[k].
Inverse: A[k] = X[k], B[k] = conj X[M-k] (A[0] = Re X[0], B[0] = Re X[M]);  Z'[k] = (A + B) + i conj(W_n^k) (A - B);
    z = the un-normalised inverse DFT_M(Z');  y[2p] = w[2p] Re z[p] / n;  y[2p+1] = w[2p+1] Im z[p] / n.
"""
import numpy as np

SIZES = (512, 1024, 2048, 4096, 8192)


def check_n(n):
    if n not in SIZES:
        raise ValueError(f"n must be one of {SIZES}, not {n}")
    return n


def _ctype(dtype):
    return np.complex64 if dtype == np.float32 else np.complex128


def _window(w, n, dtype=np.float64):
    return np.ones(n, dtype) if w is None else np.asarray(w).astype(dtype)


def hann(n, dtype=np.float64):
    """the periodic Hann window 0.5 - 0.5 cos(2 pi j / n), j < n (torch.hann_window(n, periodic=True))"""
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)).astype(dtype)


def direct(x, w=None):
    """X[k] = sum_j w[j] x[j] exp(-2 pi i jk / n), k <= n / 2, fp64: frames on the last axis"""
    x = np.asarray(x, np.float64)
    n = x.shape[-1]
    return (x * _window(w, n)) @ np.exp(-2j * np.pi * np.outer(np.arange(n), np.arange(n // 2 + 1)) / n)


def inverse_direct(X, w=None):
    """y[j] = w[j] (1/n) sum_{k<n} X[k] exp(2 pi i jk / n) with X[n-k] = conj X[k] and real bins 0 and n / 2, fp64"""
    X = np.asarray(X, np.complex128)
    M = X.shape[-1] - 1
    n = 2 * M
    full = np.concatenate([X[..., :1].real, X[..., 1:M], X[..., M:].real, np.conj(X[..., M - 1:0:-1])], axis=-1)
    y = (full @ np.exp(2j * np.pi * np.outer(np.arange(n), np.arange(n)) / n)).real / n
    return y * _window(w, n)


def twiddles(n, dtype):
    """W_n^k = exp(-2 pi i k / n), k < M, of the precision of dtype: fp64 values rounded once"""
    return np.exp(-2j * np.pi * np.arange(n // 2) / n).astype(_ctype(dtype))


def chain(x, w=None, dtype=np.float64, power=False):
    """the forward kernel: frames of n samples on the last axis -> M + 1 complex bins (or their powers)"""
    x = np.asarray(x)
    n = check_n(x.shape[-1])
    M = n // 2
    ct = _ctype(dtype)
    v = x.astype(dtype) if w is None else (x.astype(dtype) * _window(w, n, dtype)).astype(dtype)
    z = (v[..., 0::2] + 1j * v[..., 1::2]).astype(ct)
    Z = np.fft.fft(z.astype(np.complex128), axis=-1).astype(ct)
    P = np.conj(np.roll(Z[..., ::-1], 1, axis=-1))                    # conj Z[(M - k) mod M]
    W = twiddles(n, dtype)
    X = np.empty(x.shape[:-1] + (M + 1,), ct)
    X[..., :M] = (0.5 * ((Z + P).astype(ct) - 1j * (W * (Z - P).astype(ct)).astype(ct))).astype(ct)
    X[..., 0] = (Z[..., 0].real + Z[..., 0].imag).astype(dtype)
    X[..., M] = (Z[..., 0].real - Z[..., 0].imag).astype(dtype)
    if power:
        return (X.real.astype(dtype) ** 2 + X.imag.astype(dtype) ** 2).astype(dtype)
    return X


def inverse_chain(X, w=None, dtype=np.float64):
    """the inverse kernel: rows of M + 1 complex bins on the last axis -> n windowed samples"""
    X = np.asarray(X)
    M = X.shape[-1] - 1
    n = check_n(2 * M)
    ct = _ctype(dtype)
    X = X.astype(ct)
    A = X[..., :M].copy()
    B = np.conj(X[..., M:0:-1])                                       # conj X[M - k]
    A[..., 0] = A[..., 0].real
    B[..., 0] = B[..., 0].real
    W = np.conj(twiddles(n, dtype))
    Zp = ((A + B).astype(ct) + 1j * (W * (A - B).astype(ct)).astype(ct)).astype(ct)
    z = (np.fft.ifft(Zp.astype(np.complex128), axis=-1) * M).astype(ct)
    y = np.empty(X.shape[:-1] + (n,), dtype)
    y[..., 0::2] = z.real / dtype(n)
    y[..., 1::2] = z.imag / dtype(n)
    return y if w is None else (y * _window(w, n, dtype)).astype(dtype)


def frames(s, n, hop):
    """(..., L) -> (..., 1 + (L - n) // hop, n): the frames of n samples at hop"""
    s = np.asarray(s)
    F = 1 + (s.shape[-1] - n) // hop
    return np.stack([s[..., f * hop:f * hop + n] for f in range(F)], axis=-2)


def overlap_add(y, hop, w=None, length=None):
    """(..., F, n) -> (..., (F - 1) hop + n), cut or padded to length: frame f added at offset f hop; with a window, divided by the sum
    of its squares at the same offsets (which must stay above 1e-11: torch.istft's rule)"""
    y = np.asarray(y)
    F, n = y.shape[-2], y.shape[-1]
    out = np.zeros(y.shape[:-2] + ((F - 1) * hop + n,), y.dtype)
    for f in range(F):
        out[..., f * hop:f * hop + n] += y[..., f, :]
    if w is not None:
        env = np.zeros((F - 1) * hop + n, np.float64)
        for f in range(F):
            env[f * hop:f * hop + n] += np.asarray(w, np.float64) ** 2
        if length is not None:
            env = env[:length]
        if env.min() < 1e-11:
            raise ValueError("the window's overlap-add envelope falls below 1e-11")
        out = out[..., :env.shape[0]] / env.astype(y.dtype)
    if length is not None:
        out = out[..., :length] if out.shape[-1] >= length else np.concatenate([out, np.zeros(out.shape[:-1] + (length - out.shape[-1],), out.dtype)], axis=-1)
    return out


def errors(got, want):
    """(worst row relL2, worst row max |d| / max |want|) of rows on the last axis (real or complex)"""
    got, want = np.asarray(got), np.asarray(want)
    wide = np.complex128 if np.iscomplexobj(got) or np.iscomplexobj(want) else np.float64
    got, want = got.astype(wide).reshape(-1, got.shape[-1]), want.astype(wide).reshape(-1, want.shape[-1])
    d = got - want
    l2 = np.linalg.norm(d, axis=1) / np.maximum(np.linalg.norm(want, axis=1), 1e-300)
    mx = np.max(np.abs(d), axis=1) / np.maximum(np.max(np.abs(want), axis=1), 1e-300)
    return float(l2.max()), float(mx.max())

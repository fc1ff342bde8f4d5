"""The fp64 model of the polyphase filter bank channelizer for real streams (include/smfft_pfb_real.h).

  pfb_real(x, h, N)          the definition's first form: frames of 2N samples by sliding_window_view, weighted sum over the P branches,
                             np.fft.rfft -> (C, F, N + 1)
  pfb_real_direct(x, h, N)   the second form: the O(P N^2) direct sum  sum_m h[m] x[2 f N + m] exp(-2 pi i k m / 2N), 0 <= k <= N
  pack(X)                    (..., N + 1) -> (..., N) as the device writes it: element 0 = (X[0], X[N])
  power(X)                   (..., N + 1) -> (..., N): |X[k]|^2, k < N (element 0 = X[0]^2; the Nyquist power is not output)
  scale(x, h, N)             s[c, f, n] = sum_p |h[2 p N + n]| |x_c[(f + p) 2N + n]|, n < 2N: what the fp32 accumulation rounds at

The plan is the complex bank's (tools/pfb_model.py: Plan(L / 2, N, P, C) in pairs of samples).  The CPU test ties this model to
pfb_model.pfb(x + 0j, h, 2N); the GPU tests use pfb_real() as their reference."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view


def frames(L, N, P):
    return max(L // (2 * N) - P + 1, 0)


def weighted(x, h, N):
    """(C, F, 2N): w[c, f, n] = sum_p h[2 p N + n] x_c[(f + p) 2N + n]"""
    x = np.atleast_2d(np.asarray(x, np.float64))
    h = np.asarray(h, np.float64)
    M = 2 * N
    P = h.size // M
    assert h.size == P * M and P >= 1
    C, L = x.shape
    F = frames(L, N, P)
    if F == 0:
        return np.empty((C, 0, M))
    blocks = x[:, :(F + P - 1) * M].reshape(C, F + P - 1, M)
    win = sliding_window_view(blocks, P, axis=1)          # (C, F, 2N, P): win[c, f, n, p] = x_c[(f + p) 2N + n]
    return np.einsum("cfnp,pn->cfn", win, h.reshape(P, M))


def pfb_real(x, h, N):
    """x: (C, L) real, h: P 2N real -> (C, F, N + 1) complex128, np.fft.rfft layout"""
    return np.fft.rfft(weighted(x, h, N), axis=-1)


def pfb_real_direct(x, h, N):
    x = np.atleast_2d(np.asarray(x, np.float64))
    h = np.asarray(h, np.float64)
    M = h.size
    P = M // (2 * N)
    C, L = x.shape
    F = frames(L, N, P)
    k, m = np.arange(N + 1)[:, None], np.arange(M)[None, :]
    E = np.exp(-2j * np.pi * ((k * m) % (2 * N)) / (2 * N))           # (N + 1, M)
    y = np.empty((C, F, N + 1), np.complex128)
    for c in range(C):
        for f in range(F):
            y[c, f] = E @ (h * x[c, 2 * f * N:2 * f * N + M])
    return y


def pack(X):
    """(..., N + 1) rfft rows -> (..., N): X[k] for 1 <= k < N, element 0 = (Re X[0], Re X[N])"""
    X = np.asarray(X)
    out = X[..., :-1].copy()
    out[..., 0] = X[..., 0].real + 1j * X[..., -1].real
    return out


def power(X):
    """(..., N + 1) rfft rows -> (..., N): |X[k]|^2 for k < N (element 0 = X[0]^2, X[0] being real)"""
    X = np.asarray(X)[..., :-1]
    return X.real ** 2 + X.imag ** 2


def scale(x, h, N):
    """s[c, f, n] = sum_p |h[2 p N + n]| |x_c[(f + p) 2N + n]|, n < 2N: the tolerances' denominator"""
    return weighted(np.abs(np.atleast_2d(x)), np.abs(np.asarray(h, np.float64)), N)

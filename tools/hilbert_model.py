"""NumPy model of the chain of libsmfft_hilbert.so (smfft_amd/csrc/smfft_hilbert.hip): the Hilbert transform, the analytic signal and
the envelope of rows of n points through TWO complex transforms of M = n / 2 points per row.

    direct(x, kind)                  the definition in fp64 through the full-length DFT: H(x) = IDFT_n(-i s[k] DFT_n(x)[k]),
                                     s = +1 (0 < k < n/2), -1 (n/2 < k < n), 0 (k = 0, n/2): the reference of the reference
    chain(x, kind, dtype)            the kernel's steps; dtype=np.float64: the fp64 reference of the GPU tests; np.float32: every stage
                                     rounded to fp32, the transforms themselves in fp64 and rounded once (so the model is a floor, not a
                                     bound)
    errors(got, want, x)             the two error measures of the tests, per row relative to the INPUT row: ||H(x)|| <= ||x||, and a
                                     row dominated by its mean has a small output

Kinds: 0 H(x) (float), 1 x + i H(x) (complex), 2 sqrt(x^2 + H(x)^2) (float).
Chain: z[p] = x[2p] + i x[2p+1], Z = DFT_M(z), P[k] = conj Z[(M-k) % M], W = W_n^k = c - i s,
Z'[k] = (conj(W) (Z + P) - W (Z - P)) / n = (2 / n) (c P + i s Z), Z'[0] = 0, z' = M IDFT_M(Z'), H[2p] = Re z'[p], H[2p+1] = Im z'[p].
"""
import numpy as np

SIZES = (512, 1024, 2048, 4096, 8192)
QUADRATURE, ANALYTIC, ENVELOPE = 0, 1, 2


def check_n(n):
    if n not in SIZES:
        raise ValueError(f"n must be one of {SIZES}, not {n}")
    return n


def _output(x, h, kind):
    if kind == QUADRATURE:
        return h
    if kind == ANALYTIC:
        return x + 1j * h
    if kind == ENVELOPE:
        return np.sqrt(x * x + h * h)
    raise ValueError("kind must be 0, 1 or 2")


def direct(x, kind=QUADRATURE):
    """the definition, fp64: rows on the last axis"""
    x = np.asarray(x, np.float64)
    n = x.shape[-1]
    s = np.zeros(n)
    s[1:n // 2] = 1.0
    s[n // 2 + 1:] = -1.0
    h = np.fft.ifft(-1j * s * np.fft.fft(x, axis=-1), axis=-1).real
    return _output(x, h, kind)


def chain(x, kind=QUADRATURE, dtype=np.float64):
    x = np.asarray(x)
    n = check_n(x.shape[-1])
    if kind not in (QUADRATURE, ANALYTIC, ENVELOPE):
        raise ValueError("kind must be 0, 1 or 2")
    M = n // 2
    ctype = np.complex64 if dtype == np.float32 else np.complex128
    x = x.astype(dtype)
    k = np.arange(M)
    w = np.exp(2j * np.pi * k / n).astype(ctype)                       # (c, s): the conjugate of W_n^k, fp64 rounded once
    c, s = w.real, w.imag
    z = (x[..., 0::2] + 1j * x[..., 1::2]).astype(ctype)
    with np.errstate(all="ignore"):
        Z = np.fft.fft(z.astype(np.complex128), axis=-1).astype(ctype)
        Pm = Z[..., (M - k) % M]                                        # Z[M - k]; P = conj of it
        scale = dtype(2.0 / n)
        re = ((c * Pm.real).astype(dtype) - (s * Z.imag).astype(dtype)).astype(dtype) * scale
        im = ((s * Z.real).astype(dtype) - (c * Pm.imag).astype(dtype)).astype(dtype) * scale
        Zp = (re + 1j * im).astype(ctype)
        Zp[..., 0] = 0
        zp = (np.fft.ifft(Zp.astype(np.complex128), axis=-1) * M).astype(ctype)
        h = np.empty(x.shape, dtype)
        h[..., 0::2] = zp.real
        h[..., 1::2] = zp.imag
        out = _output(x, h, kind)
    return out.astype(ctype if kind == ANALYTIC else dtype)


def errors(got, want, x):
    """(worst row ||got - want||_2 / ||x||_2, worst row max |got - want| / max |x|) of rows on the last axis"""
    n = np.shape(x)[-1]
    got, want = np.asarray(got).reshape(-1, n), np.asarray(want).reshape(-1, n)
    x = np.asarray(x, np.float64).reshape(-1, n)
    d = np.abs(got.astype(np.complex128) - want)
    l2 = np.linalg.norm(d, axis=1) / np.maximum(np.linalg.norm(x, axis=1), 1e-300)
    mx = np.max(d, axis=1) / np.maximum(np.max(np.abs(x), axis=1), 1e-300)
    return float(l2.max()), float(mx.max())

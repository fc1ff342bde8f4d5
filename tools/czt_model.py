"""fp64 NumPy model of libsmfft_czt.so (smfft_amd/csrc/smfft_czt.hip, include/smfft_czt.h): the plan's three tables as the header
defines them, the kernel's chain -- multiply by the input chirp A, pad to M, FFT_M, product with the spectrum (times M: the table holds
DFT_M(b) / M and NumPy's inverse divides by M itself), IFFT_M, window to m, multiply by the output chirp C -- and `direct`, the
O(n m) sum of the definition, which is the reference of the tests (tests/test_sm_czt_cpu.py, tests/test_sm_czt_gpu.py).

Phases are formed in cycles and reduced modulo 1 before any exponential.  A product of a double s with an integer (or half of one)
q < 2^26 is taken exactly: s is split into a head of 26 bits and a tail (Veltkamp), head q and tail q are exact in fp64, and each is
reduced on its own.  What is left is the rounding of a sum of a few numbers below 1: about 1e-16 cycles.
    python tools/czt_model.py            (prints the model's distance from `direct` at a few shapes)"""
import math

import numpy as np

SIZES = (256, 512, 1024, 2048, 4096)
MAX_LENGTH = 2048


def fft_size(n, m):
    """M: the smallest of SIZES with M >= n + m - 1"""
    for name, v in (("n", n), ("m", m)):
        if not 1 <= v <= MAX_LENGTH:
            raise ValueError(f"{name} = {v} outside 1 ... {MAX_LENGTH}")
    return next(M for M in SIZES if M >= n + m - 1)


def cycles(s, q):
    """(s q) mod 1 in cycles, elementwise, to about 1e-16: s a double with |s| <= 2^500, q an array of integers or halves of integers
    below 2^26 in modulus.  The result lies in (-2, 2): a sum of two reduced parts, not reduced again"""
    s = float(s)
    q = np.asarray(q, np.float64)
    assert np.all(np.abs(q) < 2.0 ** 26) and np.all(q * 2 == np.rint(q * 2))
    c = 134217729.0 * s                   # 2^27 + 1
    head = c - (c - s)
    tail = s - head
    return np.fmod(head * q, 1.0) + np.fmod(tail * q, 1.0)


def unit(p):
    """exp(2 pi i p) of phases p in cycles, reduced to [-1/2, 1/2] first"""
    p = np.asarray(p, np.float64)
    return np.exp(2j * np.pi * (p - np.rint(p)))


def tables(n, m, start, step):
    """(A, B, C), complex128 of M each, from start reduced to [-1/2, 1/2] and step to [-1, 1] as the library reduces them:
    A[j] = exp(-2 pi i (j start + step j^2 / 2)) for j < n, C[k] = exp(-2 pi i step k^2 / 2) for k < m, zero beyond;
    B = DFT_M(b) / M with b[t mod M] = exp(+2 pi i step t^2 / 2) for -(n - 1) <= t <= m - 1 and zero elsewhere"""
    M = fft_size(n, m)
    start, step = math.remainder(start, 1.0), math.remainder(step, 2.0)
    t = np.arange(M, dtype=np.float64)
    chirp = cycles(step, 0.5 * t * t)
    A, C, b = (np.zeros(M, np.complex128) for _ in range(3))
    A[:n] = unit(-(cycles(start, t[:n]) + chirp[:n]))
    C[:m] = unit(-chirp[:m])
    b[:m] = unit(chirp[:m])
    b[M - np.arange(1, n)] = unit(chirp[1:n])
    return A, np.fft.fft(b) / M, C


def plan(n, m, start, step):
    """the plan as the library lays it out: (3M,) complex128, A then B then C"""
    return np.concatenate(tables(n, m, start, step))


def model(x, m, start, step):
    """x: (..., n) -> (..., m) complex128 by the kernel's chain in fp64"""
    x = np.asarray(x, np.complex128)
    n = x.shape[-1]
    M = fft_size(n, m)
    A, B, C = tables(n, m, start, step)
    a = np.zeros(x.shape[:-1] + (M,), np.complex128)
    a[..., :n] = x * A[:n]
    p = np.fft.ifft(np.fft.fft(a, axis=-1) * (B * M), axis=-1)
    return p[..., :m] * C[:m]


def phases(n, m, start, step):
    """(n, m) float64: j (start + k step) mod 1 in cycles, each in (-4, 4) and good to about 1e-15 -- the exponent of the definition,
    with no use of the chirp identity.  Whole cycles of start and step change nothing, since j and j k are integers; both are reduced
    (exactly) first"""
    start, step = math.remainder(start, 1.0), math.remainder(step, 1.0)
    j = np.arange(n, dtype=np.float64)
    k = np.arange(m, dtype=np.float64)
    return cycles(start, j)[:, None] + cycles(step, j[:, None] * k[None, :])


def direct(x, m, start, step):
    """x: (..., n) -> (..., m) complex128: out[..., k] = sum_j x[..., j] exp(-2 pi i j (start + k step)), the O(n m) sum in fp64"""
    x = np.asarray(x, np.complex128)
    return x @ unit(-phases(x.shape[-1], m, start, step))


if __name__ == "__main__":
    rng = np.random.default_rng(0)
    for n, m, start, step in ((1, 1, .3, .1), (128, 129, .25, 1 / 1024), (1000, 24, .123, 1e-4), (2048, 2048, 0, 1 / 2048), (300, 2048, .9, -.013),
                              (1536, 513, .4, .3)):
        x = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
        want = direct(x, m, start, step)
        got = model(x, m, start, step)
        print(f"n={n:5d} m={m:5d} M={fft_size(n, m):5d} start={start:g} step={step:g}: max |model - direct| / max |direct| = "
              f"{np.max(np.abs(got - want)) / np.max(np.abs(want)):.2e}")

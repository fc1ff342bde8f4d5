"""NumPy model of libsmfft_rowconv_real.so (smfft_amd/csrc/smfft_rowconv_real.hip, include/smfft_rowconv_real.h): `fft_size` and
`window` (those of rowconv_model.py); `direct`, the fp64 sum of the definition for both modes and the window, which is the reference of
the tests (tests/test_sm_rowconv_real_cpu.py, tests/test_sm_rowconv_real_gpu.py); `exponent_rule` and `row_exponent`, the rule by which
the kernel balances the two rows of a pair (smfft_rowconv_real_scale.hpp); and `model`, the kernel's chain -- the row exponents, both
rows scaled and packed into one complex row z = a + i b', FFT_M, the partner Z[M - k], the product S D (-i / 4M), un-normalised inverse
FFT_M, the real part scaled back, window -- in fp64 or, with dtype=np.float32, with every stage's result rounded to fp32 (NumPy's
transforms run in the precision of their input).  balance=False is the chain without the row exponents: what packing two unrelated
rows into one number system costs when their energies differ.
    python tools/rowconv_real_model.py        (prints the fp32 model's distance from `direct` per shape and scale, with and without)"""
import numpy as np

import rowconv_model
from rowconv_model import fft_size, window  # noqa: F401  (the same functions: one M per Lfull)

SIZES = rowconv_model.SIZES
MAX_FULL = rowconv_model.MAX_FULL


def second_operand(b, correlate=False):
    """(..., n_b): the row that is convolved with a: b itself, or b reversed, which turns the correlation into a convolution"""
    b = np.asarray(b)
    return b[..., ::-1] if correlate else b


def direct(a, b, correlate=False, first=0, m=None):
    """a: (..., n_a), b: (..., n_b), real -> (..., m) float64: elements first ... first + m - 1 of y[k] = sum_j a[j] b[k - j] (convolve)
    or y[k] = sum_j a[j + k - (n_b - 1)] b[j] (correlate), summed in fp64 term by term (rowconv_model.direct on the real rows)"""
    a, b = np.asarray(a), np.asarray(b)
    if np.iscomplexobj(a) or np.iscomplexobj(b):
        raise TypeError("real rows only")
    return np.ascontiguousarray(rowconv_model.direct(a.astype(np.float64), b.astype(np.float64), correlate, first, m).real)


def ilogb(x):
    """the exponent of the leading one of positive finite x (an array): floor(log2(x)), exact, subnormals included"""
    return np.frexp(x)[1].astype(np.int64) - 1


def exponent_rule(mx, s):
    """(k, zero, finite) from a row's largest magnitude mx and s = sum_j ldexp(x_j, -ilogb(mx))^2, as smfft::rowconv_real::row_scale
    has it: k = -ilogb(mx) - floor(ilogb(s) / 2); k = 0 for a row of zeros (zero) and for one with an Inf or a NaN (not finite), whose s
    is not looked at"""
    mx, s = np.abs(np.asarray(mx, np.float32)), np.abs(np.asarray(s, np.float32))
    zero = mx == 0
    finite = np.isfinite(mx)
    plain = finite & ~zero
    p = ilogb(np.where(plain, mx, np.float32(1)))
    e = ilogb(np.where(plain & np.isfinite(s) & (s > 0), s, np.float32(1)))
    return np.where(plain, -p - (e >> 1), 0), zero, finite


def row_exponent(x):
    """x: (..., n) float32 -> (k, zero, finite) per row: ldexp(x, k) has its sum of squares in [1, 4)"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        mx = np.max(np.abs(x), axis=-1)
        mx = np.where(np.isnan(x).any(axis=-1), np.float32(np.nan), mx)
        plain = np.isfinite(mx) & (mx != 0)
        p = ilogb(np.where(plain, mx, np.float32(1)))
        scaled = np.ldexp(x, (-p)[..., None].astype(np.int32)).astype(np.float32)
        s = np.sum(scaled * scaled, axis=-1, dtype=np.float32)
    return exponent_rule(mx, s)


def model(a, b, correlate=False, first=0, m=None, dtype=np.float64, balance=True):
    """the kernel's chain in the precision of dtype (np.float64, or np.float32 for an fp32 model of the kernel's rounding)"""
    real = np.dtype(dtype).type
    cplx = np.complex64 if real == np.float32 else np.complex128
    a, b = np.asarray(a, real), np.asarray(b, real)
    n_a, n_b = a.shape[-1], b.shape[-1]
    M = fft_size(n_a, n_b)
    first, m = window(n_a, n_b, first, m)
    lead = np.broadcast_shapes(a.shape[:-1], b.shape[:-1])
    ka = kb = np.zeros(lead, np.int64)
    zero, finite = np.zeros(lead, bool), np.ones(lead, bool)
    if balance:
        (ka, za, fa), (kb, zb, fb) = row_exponent(a), row_exponent(b)
        zero, finite = za | zb, fa & fb
    with np.errstate(invalid="ignore", over="ignore"):
        z = np.zeros(lead + (M,), cplx)
        z[..., :n_a].real = np.ldexp(a, ka[..., None].astype(np.int32))
        z[..., :n_b].imag = np.ldexp(second_operand(b, correlate), kb[..., None].astype(np.int32))
        Z = np.fft.fft(z, axis=-1).astype(cplx)
        P = np.conj(Z[..., (-np.arange(M)) % M])
        S, D = (Z + P).astype(cplx), (Z - P).astype(cplx)
        C = ((S * D).astype(cplx) * cplx(-0.25j / M)).astype(cplx)
        y = (np.fft.ifft(C, axis=-1).astype(cplx).real * real(M)).astype(real)
        y = np.ldexp(y, (-(ka + kb))[..., None].astype(np.int32)).astype(real)
        y = np.where(zero[..., None], y * real(0) + real(0), y + real(0))
        y = np.where(finite[..., None], y, real(np.nan))
    return y[..., first:first + m]


def errors(got, want):
    """(worst row relL2, worst row max |d| / max |want|)"""
    d = got.astype(np.float64) - want
    return (float(np.max(np.linalg.norm(d, axis=-1) / np.linalg.norm(want, axis=-1))),
            float(np.max(np.max(np.abs(d), axis=-1) / np.max(np.abs(want), axis=-1))))


SHAPES = ((1, 1), (1, 256), (256, 1), (128, 129), (129, 129), (300, 200), (200, 300), (1000, 25), (1000, 26), (4095, 2), (2, 4095), (4096, 1),
          (1, 4096), (2048, 2049), (1536, 513))

if __name__ == "__main__":
    rng = np.random.default_rng(0)
    for n_a, n_b in SHAPES:
        a = rng.standard_normal((3, n_a)).astype(np.float32)
        b0 = rng.standard_normal((3, n_b)).astype(np.float32)
        for s in (0, -12, 12, -60, 60):
            b = np.ldexp(b0, s).astype(np.float32)
            for correlate in (False, True):
                want = direct(a, b, correlate)
                with_k, without = errors(model(a, b, correlate, dtype=np.float32), want), errors(model(a, b, correlate, dtype=np.float32, balance=False), want)
                print(f"n_a={n_a:5d} n_b={n_b:5d} M={fft_size(n_a, n_b):5d} b * 2^{s:<3d} {'correlate' if correlate else 'convolve '}: fp32 model relL2 = "
                      f"{with_k[0]:.2e}, max |d| / max |want| = {with_k[1]:.2e}; without the balancing {without[0]:.2e}, {without[1]:.2e}")

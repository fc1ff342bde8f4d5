"""NumPy model of libsmfft_rowconv.so (smfft_amd/csrc/smfft_rowconv.hip, include/smfft_rowconv.h): `fft_size`; `direct`, the fp64
sum of the definition for both modes and the window, which is the reference of the tests (tests/test_sm_rowconv_cpu.py,
tests/test_sm_rowconv_gpu.py); `second_operand`, the row the kernel convolves with (b, or conj(b) reversed); and `model`, the kernel's
chain -- pad both rows to M, scale the second operand by 1 / M, FFT_M of each, product, un-normalised inverse FFT_M, window -- in fp64
or, with dtype=np.complex64, with every stage's result rounded to fp32 (NumPy's transforms run in the precision of their input).
    python tools/rowconv_model.py        (prints the fp32 model's distance from `direct` at a few shapes, both modes)"""
import numpy as np

SIZES = (256, 512, 1024, 2048, 4096)
MAX_FULL = 4096


def fft_size(n_a, n_b):
    """M: the smallest of SIZES with M >= n_a + n_b - 1"""
    if n_a < 1 or n_b < 1 or n_a + n_b - 1 > MAX_FULL:
        raise ValueError(f"n_a = {n_a}, n_b = {n_b}: outside n_a, n_b >= 1, n_a + n_b - 1 <= {MAX_FULL}")
    return next(M for M in SIZES if M >= n_a + n_b - 1)


def window(n_a, n_b, first=0, m=None):
    """(first, m) checked against the full length n_a + n_b - 1; m = the rest of the full result when None"""
    full = n_a + n_b - 1
    m = full - first if m is None else m
    if first < 0 or m < 1 or first + m > full:
        raise ValueError(f"first = {first}, m = {m}: outside 0 <= first, 1 <= m, first + m <= {full}")
    return first, m


def second_operand(b, correlate=False):
    """(..., n_b): the row that is convolved with a: b itself, or conj(b) reversed, which turns the correlation into a convolution"""
    b = np.asarray(b)
    return np.conj(b[..., ::-1]) if correlate else b


def direct(a, b, correlate=False, first=0, m=None):
    """a: (..., n_a), b: (..., n_b) -> (..., m) complex128: elements first ... first + m - 1 of
    y[k] = sum_j a[j] b[k - j] (convolve) or y[k] = sum_j a[j + k - (n_b - 1)] conj(b[j]) (correlate), summed in fp64 term by term:
    shifted copies of the longer row, each scaled by one element of the shorter one"""
    a, b = np.asarray(a, np.complex128), np.asarray(b, np.complex128)
    n_a, n_b = a.shape[-1], b.shape[-1]
    fft_size(n_a, n_b)
    first, m = window(n_a, n_b, first, m)
    h = second_operand(b, correlate)
    y = np.zeros(np.broadcast_shapes(a.shape[:-1], b.shape[:-1]) + (n_a + n_b - 1,), np.complex128)
    long, short = (a, h) if n_a >= n_b else (h, a)      # the convolution commutes: the loop runs over the shorter row
    for e in range(short.shape[-1]):
        y[..., e:e + long.shape[-1]] += long * short[..., e:e + 1]
    return y[..., first:first + m]


def model(a, b, correlate=False, first=0, m=None, dtype=np.complex128):
    """the kernel's chain in the precision of dtype (np.complex128, or np.complex64 for an fp32 model of the kernel's rounding)"""
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    n_a, n_b = a.shape[-1], b.shape[-1]
    M = fft_size(n_a, n_b)
    first, m = window(n_a, n_b, first, m)
    real = np.float32 if dtype == np.complex64 else np.float64
    pa = np.zeros(a.shape[:-1] + (M,), dtype)
    pb = np.zeros(b.shape[:-1] + (M,), dtype)
    pa[..., :n_a] = a
    pb[..., :n_b] = second_operand(b, correlate) * real(1.0 / M)
    spectrum = (np.fft.fft(pa, axis=-1).astype(dtype) * np.fft.fft(pb, axis=-1).astype(dtype)).astype(dtype)
    y = (np.fft.ifft(spectrum, axis=-1) * real(M)).astype(dtype)
    return y[..., first:first + m]


if __name__ == "__main__":
    rng = np.random.default_rng(0)
    for n_a, n_b in ((1, 1), (128, 129), (300, 200), (1000, 25), (2048, 2049), (4095, 2), (1, 4096), (1536, 513)):
        a = (rng.standard_normal((3, n_a)) + 1j * rng.standard_normal((3, n_a))).astype(np.complex64)
        b = (rng.standard_normal((3, n_b)) + 1j * rng.standard_normal((3, n_b))).astype(np.complex64)
        for correlate in (False, True):
            want = direct(a, b, correlate)
            got = model(a, b, correlate, dtype=np.complex64)
            d = got - want
            print(f"n_a={n_a:5d} n_b={n_b:5d} M={fft_size(n_a, n_b):5d} {'correlate' if correlate else 'convolve '}: fp32 model relL2 = "
                  f"{np.max(np.linalg.norm(d, axis=-1) / np.linalg.norm(want, axis=-1)):.2e}, max |d| / max |want| = "
                  f"{np.max(np.max(np.abs(d), axis=-1) / np.max(np.abs(want), axis=-1)):.2e}")

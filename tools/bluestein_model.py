"""fp64 NumPy model of libsmfft_bluestein.so (smfft_amd/csrc/smfft_bluestein.hip, include/smfft_bluestein.h): the plan's two tables as
the header defines them, and the kernel's chain -- multiply by the chirp, pad to M, FFT_M, product with the spectrum (times M: the
table holds DFT_M(b) / M and NumPy's inverse divides by M itself), IFFT_M, window to n, multiply by the chirp -- which is np.fft.fft
(inverse: np.fft.ifft * n) to fp64 rounding (tests/test_sm_bluestein_cpu.py).
    python tools/bluestein_model.py            (prints the model's distance from np.fft at a few lengths)"""
import numpy as np

SIZES = (256, 512, 1024, 2048, 4096)
MAX_LENGTH = 2048


def fft_size(n):
    """M: the smallest of SIZES with M >= 2n - 1"""
    if not 1 <= n <= MAX_LENGTH:
        raise ValueError(f"n = {n} outside 1 ... {MAX_LENGTH}")
    return next(m for m in SIZES if m >= 2 * n - 1)


def tables(n, inverse=False):
    """(W, B), complex128 of M each: W[j] = exp(-+ i pi (j^2 mod 2n) / n) for j < n and zero beyond; B = DFT_M(b) / M with
    b[j] = conj(W[j]) for j < n, b[M - j] = b[j] for 1 <= j < n and zero elsewhere"""
    M = fft_size(n)
    j = np.arange(n, dtype=np.int64)
    angle = np.pi * ((j * j) % (2 * n)).astype(np.float64) / n
    W = np.zeros(M, np.complex128)
    W[:n] = np.cos(angle) + (1j if inverse else -1j) * np.sin(angle)
    b = np.zeros(M, np.complex128)
    b[:n] = np.conj(W[:n])
    b[M - j[1:]] = b[j[1:]]
    return W, np.fft.fft(b) / M


def plan(n, inverse=False):
    """the plan as the library lays it out: (2M,) complex128, W then B"""
    return np.concatenate(tables(n, inverse))


def model(x, n, inverse=False):
    """x: (..., n) -> (..., n) complex128 by the kernel's chain in fp64"""
    x = np.asarray(x, np.complex128)
    assert x.shape[-1] == n
    M = fft_size(n)
    W, B = tables(n, inverse)
    a = np.zeros(x.shape[:-1] + (M,), np.complex128)
    a[..., :n] = x * W[:n]
    p = np.fft.ifft(np.fft.fft(a, axis=-1) * (B * M), axis=-1)
    return p[..., :n] * W[:n]


if __name__ == "__main__":
    rng = np.random.default_rng(0)
    for n in (1, 3, 128, 129, 1000, 1536, 2039, 2048):
        x = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
        for inverse in (False, True):
            want = np.fft.ifft(x, axis=-1) * n if inverse else np.fft.fft(x, axis=-1)
            got = model(x, n, inverse)
            print(f"n={n:5d} M={fft_size(n):5d} {'inverse' if inverse else 'forward'}: max |model - numpy| / max |numpy| = "
                  f"{np.max(np.abs(got - want)) / np.max(np.abs(want)):.2e}")

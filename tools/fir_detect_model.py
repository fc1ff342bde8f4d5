"""fp64 NumPy model of the detected outputs of the overlap-save FIR filter banks (smfft_amd/csrc/smfft_fir_detect.hip,
include/smfft_fir_detect.h), on the plan of tools/fir_plan_model.py: the power |y|^2 of every filter from the kernel's segmentation, and
per output sample the largest power over the filters with the filter that gave it, found as the kernel finds it -- one pass over the
filters in order with take = p > best or (p is NaN and best is not), the first filter always taking.  That rule is np.max / np.argmax
along the filter axis, NaN included (tests/test_fir_detect_cpu.py).
    python tools/fir_detect_model.py            (prints a small case against |np.convolve|^2 and np.max / np.argmax)"""
import numpy as np

import fir_plan_model as fm

SIZES = fm.SIZES


def power(x, taps, N, correlate=False):
    """x: (C, L) or (L,), taps: (K, M) or (M,) -> (C, K, L) float64: |y|^2 of the overlap-save run"""
    y = fm.overlap_save(x, taps, N, correlate)
    return y.real * y.real + y.imag * y.imag


def direct_power(x, taps, correlate=False):
    """the definition: |np.convolve|^2 or |np.correlate|^2"""
    y = fm.direct(x, taps, correlate)
    return y.real * y.real + y.imag * y.imag


def running_peak(p):
    """p: (C, K, L) powers -> ((C, L) best, (C, L) int32 index) by the kernel's loop over the filters"""
    p = np.asarray(p)
    best = p[:, 0].copy()
    index = np.zeros(best.shape, np.int32)
    for k in range(1, p.shape[1]):
        v = p[:, k]
        with np.errstate(invalid="ignore"):
            take = (v > best) | (np.isnan(v) & ~np.isnan(best))
        best = np.where(take, v, best)
        index = np.where(take, np.int32(k), index)
    return best, index


def peak(x, taps, N, correlate=False):
    """-> ((C, L) float64, (C, L) int32): the largest power over the filters and the lowest filter index that attains it"""
    return running_peak(power(x, taps, N, correlate))


if __name__ == "__main__":
    rng = np.random.default_rng(0)
    N, M, L = 256, 65, 500
    x = rng.standard_normal((2, L)) + 1j * rng.standard_normal((2, L))
    h = rng.standard_normal((5, M)) + 1j * rng.standard_normal((5, M))
    for corr in (False, True):
        want = direct_power(x, h, corr)
        got = power(x, h, N, corr)
        best, index = running_peak(got)
        print(("correlate" if corr else "convolve"), f"N={N} M={M} L={L} K={h.shape[0]}: max |power - numpy| / max = "
              f"{np.max(np.abs(got - want)) / np.max(want):.2e}; peak == np.max: {np.array_equal(best, got.max(axis=1))}, "
              f"index == np.argmax: {np.array_equal(index, got.argmax(axis=1))}; filters chosen: {np.bincount(index.ravel(), minlength=h.shape[0])}")

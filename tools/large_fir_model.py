"""fp64 NumPy model of the overlap-save FIR filter banks with N = 8192 / 16384 segments (include/smfft/smfft_large_fir.hpp).

The segmentation is that of tools/fir_plan_model.py (its Window / segment / spectra, whose arithmetic does not depend on N; only its
assertion on N does, which the Window here replaces), the two transforms are tools/large_plan_model.py's replay of the single-pass
engine, and what the kernel adds is replayed per thread: thread u loads the segment's elements u + T*q, q < 16, holds X[u + T*q] after
the forward transform, multiplies by H_k[u + T*q], feeds the products to the inverse transform as its inputs u + T*c without any
exchange, and stores its outputs j = u + T*q inside the window [M - 1, store_end) at row_base + j, where row_base = s V - (M - 1) is
the one 64-bit quantity per segment.  The clamped load (address min(max(e, lo), hi - 1), zero selected when e was clamped) is replayed
with its two 32-bit bounds.  overlap_save() asserts that the store windows tile [0, L) exactly once.

    python tools/large_fir_model.py        # error against np.convolve / np.correlate at both lengths
"""
import numpy as np

import fir_plan_model as fm
import large_plan_model as lpm

SIZES = lpm.SIZES
spectra = fm.spectra
segment = fm.segment
direct = fm.direct


class Window(fm.Window):
    """fir_plan_model.Window at N = 8192 / 16384"""

    def __init__(self, L, N, M, correlate):
        assert N in SIZES and 1 <= M <= N - 1 and L >= 1
        self.L, self.N, self.M, self.correlate = int(L), int(N), int(M), bool(correlate)
        self.V = N - M + 1

    def load_bounds(self, s):
        """the elements e in [lo, hi) of segment s that lie inside the signal: the kernel's two uniform 32-bit bounds"""
        a = self.load_start(s)
        lo, hi = max(0, -a), min(self.N, self.L - a)
        assert 0 <= lo < hi <= self.N
        return lo, hi


def thread_positions(N):
    """(T, 16): the element numbers u + T*q that thread u holds at the load, the product and the store"""
    T = lpm.geometry(N)["T"]
    return np.arange(T)[:, None] + T * np.arange(16)[None, :]


def load_registers(xc, w, s):
    """thread u's sixteen loads of segment s of channel xc: from the clamped address, zero where the element was clamped"""
    pos = thread_positions(w.N)
    lo, hi = w.load_bounds(s)
    ec = np.clip(pos, lo, hi - 1)
    a = w.load_start(s)
    assert (a + ec).min() >= 0 and (a + ec).max() < w.L, "a load outside the channel"
    return np.where(ec == pos, xc[a + ec], 0)


def overlap_save(x, taps, N, correlate=False):
    """x: (C, L) or (L,), taps: (K, M) or (M,) -> (C, K, L) in fp64 by the kernel's plan"""
    x = np.atleast_2d(np.asarray(x, dtype=np.complex128))
    H = spectra(taps, N, correlate)
    C, L = x.shape
    K, M = H.shape[0], np.atleast_2d(taps).shape[1]
    w = Window(L, N, M, correlate)
    pos = thread_positions(N)
    y = np.zeros((C, K, L), np.complex128)
    hits = np.zeros(L, np.int64)
    for s in range(w.segments()):
        b, e = w.store_window(s)
        row_base = w.output_index(s, 0)
        stored = (pos >= b) & (pos < e)
        hits[row_base + pos[stored]] += 1
        for c in range(C):
            regs = load_registers(x[c], w, s)
            seg = np.empty(N, np.complex128)
            seg[pos] = regs
            assert np.array_equal(seg, segment(x[c], w, s))
            X = lpm.run(seg)[pos]                      # the forward transform's output registers
            for k in range(K):
                p = np.empty(N, np.complex128)
                p[pos] = X * H[k][pos]                 # ... are the inverse transform's input registers
                out = lpm.run(p, inverse=True)[pos]
                y[c, k, row_base + pos[stored]] = out[stored]
    assert np.all(hits == 1), "the store windows must tile [0, L) exactly once"
    return y


def fft_size(n_taps):
    """the transform length smfft_amd.large_fir.fir picks: the next power of two >= 4 M, clamped to 8192 ... 16384"""
    assert 1 <= n_taps < 16384
    return min(16384, max(8192, 1 << (4 * n_taps - 1).bit_length()))


if __name__ == "__main__":
    rng = np.random.default_rng(0)
    for N in SIZES:
        M, L = N // 4 + 1, 2 * N
        x = rng.standard_normal((1, L)) + 1j * rng.standard_normal((1, L))
        h = rng.standard_normal((2, M)) + 1j * rng.standard_normal((2, M))
        for corr in (False, True):
            ref = direct(x, h, corr)
            err = np.max(np.abs(overlap_save(x, h, N, corr) - ref)) / np.max(np.abs(ref))
            print(f"N={N} M={M} L={L} {'correlate' if corr else 'convolve'}: max |model - numpy| / max |numpy| = {err:.2e}")

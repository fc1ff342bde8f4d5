"""fp64 NumPy model of the overlap-save FIR filter banks for real signals and real taps (smfft_amd/csrc/smfft_fir_real.hpp, FirPairs;
include/smfft_fir_real.h).

The segmentation is tools/fir_plan_model.py's Window, unchanged.  For a real filter g, conv(x1 + i x2, g) = conv(x1, g) + i conv(x2, g):
two consecutive segments 2p, 2p + 1 of one channel ride in the real and the imaginary lane of one complex N-point transform.  A channel
of S segments is P = ceil(S / 2) pairs; the last pair of an odd S has no second segment (its lane is loaded as zero and never stored).
What the kernel does is replayed per thread: thread u of a transform holds the elements u + T*q, q < 16, T = N / 16, at the load (two
clamped loads per element, one per lane, zeroed where the element was clamped or the segment is absent), at the product with
H_k[u + T*q] and at the two stores (lane 0 at row offset output_index(2p, j), lane 1 at output_index(2p + 1, j), each inside its own
store window).  overlap_save_pairs() asserts that the store windows tile [0, L) exactly once.

    python tools/fir_real_model.py        # the pairs of a small case and the model's error against np.convolve / np.correlate
"""
import numpy as np

import fir_plan_model as fm

SIZES = fm.SIZES
Window = fm.Window


class Pairs:
    """smfft::FirPairs: the pairs of one channel of length L under Window(L, N, M, correlate)"""

    def __init__(self, L, N, M, correlate):
        self.w = Window(L, N, M, correlate)

    def pairs(self):
        return (self.w.segments() + 1) // 2

    def segment(self, p, lane):
        return 2 * p + lane

    def present(self, p, lane):
        return self.segment(p, lane) < self.w.segments()

    def load_start(self, p, lane):
        return self.w.load_start(self.segment(p, lane))

    def store_end(self, p, lane):
        return self.w.store_window(self.segment(p, lane))[1] if self.present(p, lane) else 0

    def output_index(self, p, lane, j):
        return self.w.output_index(self.segment(p, lane), j)

    def load_bounds(self, p, lane):
        """the elements e in [lo, hi) of a present lane that lie inside the signal: the kernel's 32-bit bounds; never empty"""
        a = self.load_start(p, lane)
        lo, hi = max(0, -a), min(self.w.N, self.w.L - a)
        assert 0 <= lo < hi <= self.w.N
        return lo, hi

    def load_range(self, p):
        """[begin, end): the samples of the channel that pair p reads -- the union of its present lanes' ranges, which overlap or touch"""
        spans = [(self.load_start(p, lane) + lo, self.load_start(p, lane) + hi)
                 for lane in (0, 1) if self.present(p, lane) for lo, hi in [self.load_bounds(p, lane)]]
        assert len(spans) == 1 or spans[1][0] <= spans[0][1]
        return spans[0][0], spans[-1][1]

    def store_range(self, p):
        """[begin, end): the outputs of the row that pair p writes"""
        last = 1 if self.present(p, 1) else 0
        return self.output_index(p, 0, self.w.M - 1), self.output_index(p, last, self.store_end(p, last) - 1) + 1


def thread_positions(N):
    """(T, 16): the element numbers u + T*q that thread u holds at the load, the product and the store"""
    T = N // 16
    return np.arange(T)[:, None] + T * np.arange(16)[None, :]


def load_registers(xc, pr, p):
    """the (T, 16) complex registers of pair p of the real channel xc: per lane a load from the clamped address, zero where the element
    was clamped; an absent lane borrows lane 0's addresses and is zeroed whole"""
    pos = thread_positions(pr.w.N)
    lanes = []
    for lane in (0, 1):
        src = lane if pr.present(p, lane) else 0
        lo, hi = pr.load_bounds(p, src)
        a = pr.load_start(p, src)
        ec = np.clip(pos, lo, hi - 1)
        assert (a + ec).min() >= 0 and (a + ec).max() < pr.w.L, "a load outside the channel"
        lanes.append(np.where((ec == pos) & pr.present(p, lane), xc[a + ec], 0.0))
    return lanes[0] + 1j * lanes[1]


def spectra(taps, N, correlate):
    """the prepared spectra of real taps: H_k = DFT_N(pad_N(g_k)) / N, g_k = h_k or h_k[::-1] (fir_plan_model.spectra on real input)"""
    taps = np.asarray(taps)
    assert not np.iscomplexobj(taps), "the pairing needs real taps"
    return fm.spectra(taps, N, correlate)


def overlap_save_pairs(x, taps, N, correlate=False):
    """x: (C, L) or (L,) real, taps: (K, M) or (M,) real -> (C, K, L) float64 by the kernel's plan: load, product and the two stores"""
    x = np.atleast_2d(np.asarray(x))
    assert not np.iscomplexobj(x), "the pairing needs a real signal"
    x = x.astype(np.float64)
    H = spectra(taps, N, correlate)
    C, L = x.shape
    K, M = H.shape[0], np.atleast_2d(taps).shape[1]
    pr = Pairs(L, N, M, correlate)
    pos = thread_positions(N)
    y = np.zeros((C, K, L), np.float64)
    hits = np.zeros(L, np.int64)
    for p in range(pr.pairs()):
        windows = []
        for lane in (0, 1):
            stored = (pos >= M - 1) & (pos < pr.store_end(p, lane))
            base = pr.output_index(p, lane, 0)
            hits[base + pos[stored]] += 1
            windows.append((stored, base))
        for c in range(C):
            seg = np.empty(N, np.complex128)
            seg[pos] = load_registers(x[c], pr, p)
            X = np.fft.fft(seg)[pos]                       # the forward transform's output registers
            for k in range(K):
                prod = np.empty(N, np.complex128)
                prod[pos] = X * H[k][pos]                  # ... are the inverse transform's input registers
                out = (np.fft.ifft(prod) * N)[pos]
                for lane, (stored, base) in enumerate(windows):
                    y[c, k, base + pos[stored]] = (out.real, out.imag)[lane][stored]
    assert np.all(hits == 1), "the store windows must tile [0, L) exactly once"
    return y


def nan_footprint(L, N, M, correlate, n):
    """the outputs of a row that a NaN at sample n of its channel reaches: a boolean (L,), true on the store ranges of the pairs whose
    load range contains n"""
    pr = Pairs(L, N, M, correlate)
    hit = np.zeros(L, bool)
    for p in range(pr.pairs()):
        b, e = pr.load_range(p)
        if b <= n < e:
            ob, oe = pr.store_range(p)
            hit[ob:oe] = True
    return hit


def tiles(L, C, N, M):
    """workgroup tiles of a launch: 4096 / N pairs each"""
    return -(-Pairs(L, N, M, False).pairs() * C // (4096 // N))


def fft_size(n_taps):
    """the transform length smfft_amd.fir_real.fir picks: the next power of two >= 4 M, clamped to 256 ... 4096"""
    assert 1 <= n_taps < 4096
    return min(4096, max(256, 1 << (4 * n_taps - 1).bit_length()))


direct = fm.direct

if __name__ == "__main__":
    rng = np.random.default_rng(0)
    N, M, L = 256, 65, 900
    x, h = rng.standard_normal((2, L)), rng.standard_normal((3, M))
    for corr in (False, True):
        pr = Pairs(L, N, M, corr)
        print(("correlate" if corr else "convolve"), f"N={N} M={M} L={L} V={pr.w.V} S={pr.w.segments()} P={pr.pairs()}")
        for p in range(pr.pairs()):
            second = f"{2 * p + 1}" if pr.present(p, 1) else "none"
            print(f"  pair {p}: segments {2 * p} and {second}, loads x[{pr.load_range(p)[0]}, {pr.load_range(p)[1]}), stores n in [{pr.store_range(p)[0]}, {pr.store_range(p)[1]})")
        ref = direct(x, h, corr).real
        print(f"  max |pairs - numpy| / max |numpy| = {np.max(np.abs(overlap_save_pairs(x, h, N, corr) - ref)) / np.max(np.abs(ref)):.2e}")

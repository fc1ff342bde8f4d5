"""fp64 NumPy model of the overlap-save FIR filter banks (smfft_amd/csrc/smfft_fir.hpp, FirWindow; include/smfft.h "FIR filter banks"):
the segmentation -- segment count, load start, store window, output index per segment, for both modes -- and overlap-save run with
np.fft on exactly those windows.  It equals np.convolve / np.correlate up to fp64 rounding (tests/test_fir_cpu.py).
    python tools/fir_plan_model.py            (prints the windows of a small case and the model's error against NumPy)"""
import numpy as np

SIZES = (256, 512, 1024, 2048, 4096)


class Window:
    """the segmentation of one channel of length L by filters of M taps at transform length N"""

    def __init__(self, L, N, M, correlate):
        assert N in SIZES and 1 <= M <= N - 1 and L >= 1
        self.L, self.N, self.M, self.correlate = int(L), int(N), int(M), bool(correlate)
        self.V = N - M + 1                                          # new outputs per segment

    def segments(self):
        return -(-self.L // self.V)

    def load_start(self, s):
        """segment s is x[a + e], e < N, zero outside [0, L)"""
        return s * self.V - (0 if self.correlate else self.M - 1)

    def store_window(self, s):
        """the elements j in [begin, end) of segment s that are outputs: the circular convolution with g is the linear one for
        j >= M - 1, and element j is output n = s V + j - (M - 1), which must be < L"""
        return self.M - 1, min(self.N, self.L - s * self.V + self.M - 1)

    def output_index(self, s, j):
        return s * self.V + j - (self.M - 1)


def spectra(taps, N, correlate):
    """the prepared spectra: H_k = DFT_N(pad_N(g_k)) / N, g_k = h_k or conj(h_k[::-1])"""
    h = np.atleast_2d(np.asarray(taps, dtype=np.complex128))
    g = np.conj(h[:, ::-1]) if correlate else h
    pad = np.zeros((h.shape[0], N), np.complex128)
    pad[:, :h.shape[1]] = g
    return np.fft.fft(pad, axis=-1) / N


def segment(x, w, s):
    """the N samples segment s reads (zero outside the signal)"""
    idx = w.load_start(s) + np.arange(w.N)
    ok = (idx >= 0) & (idx < w.L)
    seg = np.zeros(w.N, np.complex128)
    seg[ok] = x[idx[ok]]
    return seg


def overlap_save(x, taps, N, correlate=False):
    """x: (C, L) or (L,), taps: (K, M) or (M,) -> (C, K, L) in fp64, by the kernel's segmentation; asserts that the stored windows
    cover every output exactly once"""
    x = np.atleast_2d(np.asarray(x, dtype=np.complex128))
    H = spectra(taps, N, correlate)
    C, L = x.shape
    K, M = H.shape[0], np.atleast_2d(taps).shape[1]
    w = Window(L, N, M, correlate)
    y = np.zeros((C, K, L), np.complex128)
    hits = np.zeros(L, np.int64)
    for s in range(w.segments()):
        b, e = w.store_window(s)
        n = w.output_index(s, np.arange(b, e))
        hits[n] += 1
        for c in range(C):
            X = np.fft.fft(segment(x[c], w, s))
            y[c, :, n] = np.fft.ifft(X[None, :] * H, axis=-1)[:, b:e].T * N
    assert np.all(hits == 1), "the store windows must tile [0, L) exactly once"
    return y


def direct(x, taps, correlate=False):
    """the definition, with NumPy: np.convolve(x_c, h_k)[:L] or np.correlate(np.r_[x_c, zeros(M-1)], h_k, 'valid')"""
    x = np.atleast_2d(np.asarray(x, dtype=np.complex128))
    h = np.atleast_2d(np.asarray(taps, dtype=np.complex128))
    C, L = x.shape
    K, M = h.shape
    y = np.empty((C, K, L), np.complex128)
    for c in range(C):
        for k in range(K):
            if correlate:
                y[c, k] = np.correlate(np.r_[x[c], np.zeros(M - 1)], h[k], "valid")
            else:
                y[c, k] = np.convolve(x[c], h[k])[:L]
    return y


if __name__ == "__main__":
    rng = np.random.default_rng(0)
    N, M, L = 256, 65, 500
    x = rng.standard_normal((2, L)) + 1j * rng.standard_normal((2, L))
    h = rng.standard_normal((3, M)) + 1j * rng.standard_normal((3, M))
    for corr in (False, True):
        w = Window(L, N, M, corr)
        print(("correlate" if corr else "convolve"), f"N={N} M={M} L={L} V={w.V} S={w.segments()}")
        for s in range(w.segments()):
            b, e = w.store_window(s)
            print(f"  segment {s}: loads x[{w.load_start(s)}, {w.load_start(s) + N}), stores j in [{b}, {e}) -> n in [{w.output_index(s, b)}, {w.output_index(s, e)})")
        ref = direct(x, h, corr)
        print(f"  max |overlap-save - numpy| / max |numpy| = {np.max(np.abs(overlap_save(x, h, N, corr) - ref)) / np.max(np.abs(ref)):.2e}")

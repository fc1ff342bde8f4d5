"""What the tests of the overlap-save FIR filter banks share (tests/test_fir_gpu.py, test_large_fir_gpu.py, test_large_fir_hostsim.py and
the FIR cases of test_buffers_gpu.py): the signals, the fp64 reference, the row check and the sampled windows of a long output.  A plain
module: no tests, no fixtures; tests/test_fir_gpu.py's docstring derives the bounds and their denominators."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

ROW_REL_L2, ROW_MAX = 1e-6, 5e-6
GUARD = 4096                   # float2 after the output that must stay untouched
MODES = ("convolve", "correlate")


def _rand(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def _reference(x, h, correlate):
    """fp64 linear convolution / correlation by zero-padded FFTs (exact up to fp64 rounding; tests/test_fir_gpu.py checks it against
    np.convolve)"""
    x = np.asarray(x, np.complex128)
    h = np.asarray(h, np.complex128)
    C, L = x.shape
    K, M = h.shape
    g = np.conj(h[:, ::-1]) if correlate else h
    P = 1 << int(L + M - 1).bit_length()
    Y = np.fft.ifft(np.fft.fft(x, P)[:, None, :] * np.fft.fft(g, P)[None, :, :], axis=-1)
    off = M - 1 if correlate else 0
    return Y[:, :, off:off + L]


def _check_rows(got, want, what, x, h):
    """got, want: (C, K, L'); x: (C, L) the signal the rows were computed from, h: (K, M) the taps"""
    for c in range(want.shape[0]):
        xn, xm = np.linalg.norm(x[c]), np.max(np.abs(x[c]))
        for k in range(want.shape[1]):
            d = got[c, k].astype(np.complex128) - want[c, k]
            hn = np.linalg.norm(h[k])
            l2 = np.linalg.norm(d) / max(np.linalg.norm(want[c, k]), hn * xn, 1e-30)
            mx = np.max(np.abs(d)) / max(np.max(np.abs(want[c, k])), hn * xm, 1e-30)
            assert l2 <= ROW_REL_L2 and mx <= ROW_MAX, f"{what} row (c={c}, k={k}): relL2={l2:.3e} maxrel={mx:.3e}"


def _sampled_windows(sm, dout, x, h, L, starts, mode, what, W):
    C, K = x.shape[0], h.shape[0]
    M = h.shape[1]
    for c in range(C):
        for k in range(K):
            hk = h[k].astype(np.complex128)
            for n0 in starts[c]:
                got = np.empty(W, np.complex64)
                assert sm.lib.smfft_memcpy_d2h(got.ctypes.data, dout.ptr + ((c * K + k) * L + n0) * 8, W * 8) == 0
                if mode == "correlate":
                    seg = np.r_[x[c, n0:n0 + W + M - 1].astype(np.complex128), np.zeros(max(0, n0 + W + M - 1 - L))]
                    want = np.correlate(seg, hk, "valid")
                else:
                    lo = max(0, n0 - (M - 1))
                    seg = x[c, lo:n0 + W].astype(np.complex128)
                    want = np.convolve(seg, hk)[n0 - lo:n0 - lo + W]
                _check_rows(got[None, None], want[None, None], f"{what} c={c} k={k} n0={n0}", seg[None], hk[None])

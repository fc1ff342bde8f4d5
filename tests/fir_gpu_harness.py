"""What the tests of the overlap-save FIR filter banks share (tests/test_fir_gpu.py, test_real_fir_gpu.py, test_large_fir_gpu.py,
test_large_fir_hostsim.py and the FIR cases of test_buffers_gpu.py and test_probes_gpu.py): the signals, the fp64 reference, the row
check, a description of a bank with its guarded run, the launch plan restated, and the test bodies that are the same for every bank.  A
plain module: no tests, no fixtures; it needs no device itself (tests/test_fir_gpu_harness_cpu.py runs it on numpy memory);
tests/test_fir_gpu.py's docstring derives the bounds and their denominators.

Every run of Bank.run goes into an output prefilled with 0xFF (NaN) and followed by a guard of GUARD elements of 0x5A that must stay
untouched."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fir_plan_model as fm  # noqa: E402

from oracle.np_reference import MAX_ABS_TOL, REL_L2_TOL  # noqa: E402

ROW_REL_L2, ROW_MAX = 1e-6, 5e-6
GUARD = 4096                   # elements after the output that must stay untouched
MODES = ("convolve", "correlate")
GRID_CAP = 12288               # smfft_fir_kernel.hpp kFirGridCap: workgroups along the unit tiles; more tiles are grid-strided
GROUP_TARGET = 2048            # smfft_fir_kernel.hpp kFirTargetWorkgroups: the filter-group rule's target


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


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _group_plan(tiles, K):
    """(group size, grid rows) of a launch: the rule of smfft_fir.hpp fir_filter_group_size, restated"""
    groups = max(1, min(K, -(-GROUP_TARGET // tiles)))
    size = -(-K // groups)
    return size, -(-K // size)


class _Row:
    """a (channel, filter) row of a device output, as the `dout` of Bank.sampled_windows with C = K = 1"""

    def __init__(self, ptr):
        self.ptr = ptr


class Bank:
    """one FIR library behind the calls its GPU tests need.  sm: smfft_amd (its DeviceBuffer, memset, copies and synchronize);
    real: float32 signals, taps and outputs, two segments to a unit (else complex64, one); prepare, launch: the mirror's functions;
    c_benchmark: the library's *_benchmark itself; benchmark: the mirror's, where it has one"""

    def __init__(self, sm, real, prepare, launch, c_benchmark=None, benchmark=None):
        self.sm, self.real, self.prepare, self.launch, self.c_benchmark, self.benchmark = sm, real, prepare, launch, c_benchmark, benchmark
        self.dtype = np.float32 if real else np.complex64
        self.width = np.dtype(self.dtype).itemsize         # bytes per sample

    @classmethod
    def complex(cls, sm):
        """the main library's bank: sm.fir_prepare / fir_launch"""
        return cls(sm, False, sm.fir_prepare, sm.fir_launch, sm.lib.smfft_fir_benchmark)

    @classmethod
    def of_real(cls, sm, fr):
        """smfft_amd.fir_real"""
        return cls(sm, True, fr.prepare, fr.launch, fr.lib().smfft_fir_real_benchmark, fr.benchmark)

    @classmethod
    def large(cls, sm, lf):
        """smfft_amd.large_fir"""
        return cls(sm, False, lf.prepare, lf.launch, lf.lib().smfft_large_fir_benchmark, lf.benchmark)

    def rand(self, rng, shape):
        return rng.standard_normal(shape).astype(np.float32) if self.real else _rand(rng, shape)

    def units(self, L, N, M):
        """units of a channel: segments, or pairs of segments"""
        S = fm.Window(L, N, M, False).segments()
        return -(-S // 2) if self.real else S

    def length(self, units, N, M):
        """the L of `units` units per channel whose last segment holds a single output (and a real channel's last pair no partner)"""
        S = 2 * units - 1 if self.real else units
        return (S - 1) * (N - M + 1) + 1

    def tiles(self, L, C, N, M):
        """workgroup tiles of a launch at N <= 4096: 4096 / N units each"""
        return -(-self.units(L, N, M) * C // (4096 // N))

    # ---- the guarded run --------------------------------------------------------------------------------------------------------
    def prepared(self, h, N, mode):
        """the library's spectra of the taps h, (K, N) complex64 on the host"""
        sm = self.sm
        K, M = h.shape
        dh, dspec = sm.DeviceBuffer.from_host(h), sm.DeviceBuffer(K * N * 8)
        try:
            self.prepare(dh.ptr, dspec.ptr, M, K, N, mode)
            assert sm.lib.smfft_synchronize() == 0
            return dspec.to_host(np.complex64, (K, N))
        finally:
            dh.free()
            dspec.free()

    def run(self, x, h, N, mode, spectra=None, finite=True):
        """prepare + launch through the device-pointer API into a NaN-prefilled output followed by a guard region; returns the (C, K, L)
        result after checking that the guard is untouched and (finite) that no NaN of the prefill is left"""
        sm, w = self.sm, self.width
        C, L = x.shape
        K, M = h.shape
        assert x.dtype == self.dtype and h.dtype == self.dtype
        if spectra is None:
            spectra = self.prepared(h, N, mode)
        dx, dspec = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer.from_host(np.ascontiguousarray(spectra, dtype=np.complex64))
        total = C * K * L
        dout = sm.DeviceBuffer((total + GUARD) * w)
        try:
            assert sm.lib.smfft_memset(dout.ptr, 0xFF, total * w) == 0
            assert sm.lib.smfft_memset(dout.ptr + total * w, 0x5A, GUARD * w) == 0
            self.launch(dx.ptr, L, C, dspec.ptr, K, M, N, dout.ptr, mode)
            assert sm.lib.smfft_synchronize() == 0
            raw = dout.to_host(np.uint8, ((total + GUARD) * w,))
        finally:
            for b in (dx, dspec, dout):
                b.free()
        assert np.all(raw[total * w:] == 0x5A), "the kernel wrote past its output"
        out = raw[:total * w].view(self.dtype).reshape(C, K, L)
        if finite:
            assert np.all(np.isfinite(out.view(np.float32))), "outputs left unwritten"
        return out

    def sampled_windows(self, dout, x, h, L, starts, mode, what, W):
        """windows of W outputs at starts[c] of every (channel, filter) row of the device output dout against np.convolve / np.correlate
        on the matching input slice"""
        C, K = x.shape[0], h.shape[0]
        M = h.shape[1]
        wide = np.float64 if self.real else np.complex128
        for c in range(C):
            for k in range(K):
                hk = h[k].astype(wide)
                for n0 in starts[c]:
                    got = np.empty(W, self.dtype)
                    assert self.sm.lib.smfft_memcpy_d2h(got.ctypes.data, dout.ptr + ((c * K + k) * L + n0) * self.width, W * self.width) == 0
                    if mode == "correlate":
                        seg = np.r_[x[c, n0:n0 + W + M - 1].astype(wide), np.zeros(max(0, n0 + W + M - 1 - L))]
                        want = np.correlate(seg, hk, "valid")
                    else:
                        lo = max(0, n0 - (M - 1))
                        seg = x[c, lo:n0 + W].astype(wide)
                        want = np.convolve(seg, hk)[n0 - lo:n0 - lo + W]
                    _check_rows(got[None, None], want[None, None], f"{what} c={c} k={k} n0={n0}", seg[None], hk[None])

    # ---- the test bodies that are the same for every bank ------------------------------------------------------------------------
    def check_group_split(self, N, M, L, tiles=None, plan=None, K=200):
        """K filters in one launch: every row equals the K = 1 launch of its filter (the same spectrum) to the bit; sampled rows against
        fp64.  tiles, plan: what the launch is at N <= 4096 (workgroup tiles, (group size, grid rows))"""
        sm = self.sm
        assert tiles is None or (self.tiles(L, 1, N, M) == tiles and _group_plan(tiles, K) == plan)
        rng = np.random.default_rng(N)
        x, h = self.rand(rng, (1, L)), self.rand(rng, (K, M))
        for mode in MODES:
            spectra = self.prepared(h, N, mode)
            all_rows = self.run(x, h, N, mode, spectra=spectra)[0]
            dx, dspec, d1 = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer.from_host(spectra), sm.DeviceBuffer(L * self.width)
            for k in range(K):
                self.launch(dx.ptr, L, 1, dspec.ptr + k * N * 8, 1, M, N, d1.ptr, mode)
                assert sm.lib.smfft_synchronize() == 0
                assert np.array_equal(_bits(d1.to_host(self.dtype, (L,))), _bits(all_rows[k])), (mode, k)
            for b in (dx, dspec, d1):
                b.free()
            _check_rows(all_rows[None, ::37], _reference(x, h[::37], mode == "correlate"), f"K={K} N={N} {mode}", x, h[::37])

    def check_prepared_spectra(self, N, elsewhere=None):
        """the library's prepare = fft(pad(g)) / N within the per-FFT tolerances; launches on its own spectra, on NumPy-prepared ones and
        on those of elsewhere(h, N, mode) (another library's prepare) each pass the row check, and the first two agree within it"""
        rng = np.random.default_rng(3 * N)
        K = 7
        for mode in MODES:
            for M in (1, 17, N // 4 + 1, N - 1):
                h = self.rand(rng, (K, M))
                got = self.prepared(h, N, mode)
                want = fm.spectra(h, N, mode == "correlate")
                for k in range(K):
                    d = got[k] - want[k]
                    l2 = np.linalg.norm(d) / np.linalg.norm(want[k])
                    mx = np.max(np.abs(d)) / np.max(np.abs(want[k]))
                    assert l2 <= REL_L2_TOL and mx <= MAX_ABS_TOL, (mode, M, k, l2, mx)
                other = None if elsewhere is None else elsewhere(h, N, mode)
                x = self.rand(rng, (2, 3 * (N - M + 1) + 5))
                want_y = _reference(x, h, mode == "correlate")
                lib_out = self.run(x, h, N, mode)
                np_out = self.run(x, h, N, mode, spectra=want.astype(np.complex64))
                _check_rows(lib_out, want_y, f"own spectra N={N} {mode} M={M}", x, h)
                _check_rows(np_out, want_y, f"NumPy spectra N={N} {mode} M={M}", x, h)
                _check_rows(lib_out, np_out.astype(np.complex128), f"library vs NumPy spectra N={N} {mode} M={M}", x, h)
                if other is not None:
                    _check_rows(self.run(x, h, N, mode, spectra=other), want_y, f"spectra from elsewhere N={N} {mode} M={M}", x, h)

    def check_caller_stream(self, shapes, C, K, L):
        """prepare and launch on a stream from hipStreamCreate, then hipStreamSynchronize, at every (N, M) of shapes"""
        sm = self.sm
        hip = ctypes.CDLL("libamdhip64.so")
        hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
        hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
        stream = ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value
        rng = np.random.default_rng(11)
        for N, M in shapes:
            x, h = self.rand(rng, (C, L)), self.rand(rng, (K, M))
            for mode in MODES:
                dx, dh = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer.from_host(h)
                dspec, dout = sm.DeviceBuffer(K * N * 8), sm.DeviceBuffer(C * K * L * self.width)
                assert sm.lib.smfft_memset(dout.ptr, 0xFF, dout.nbytes) == 0
                assert sm.lib.smfft_synchronize() == 0
                self.prepare(dh.ptr, dspec.ptr, M, K, N, mode, stream=stream.value)
                self.launch(dx.ptr, L, C, dspec.ptr, K, M, N, dout.ptr, mode, stream=stream.value)
                assert hip.hipStreamSynchronize(stream) == 0
                _check_rows(dout.to_host(self.dtype, (C, K, L)), _reference(x, h, mode == "correlate"), f"stream N={N} {mode}", x, h)
                for b in (dx, dh, dspec, dout):
                    b.free()
        assert hip.hipStreamDestroy(stream) == 0

    def check_benchmark_form(self, N, M, K, L):
        """the library's *_benchmark adds its milliseconds to the caller's total and fills the output; so does the mirror's, if any"""
        sm = self.sm
        rng = np.random.default_rng(12)
        x, h = self.rand(rng, (1, L)), self.rand(rng, (K, M))
        dx, dspec = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer.from_host(self.prepared(h, N, "convolve"))
        dout = sm.DeviceBuffer(K * L * self.width)
        assert sm.lib.smfft_memset(dout.ptr, 0xFF, dout.nbytes) == 0
        t = ctypes.c_double(1.0)
        assert self.c_benchmark(dx.ptr, L, 1, dspec.ptr, K, M, N, 0, dout.ptr, ctypes.byref(t)) == 0
        assert t.value > 1.0
        _check_rows(dout.to_host(self.dtype, (1, K, L)), _reference(x, h, False), "benchmark form", x, h)
        if self.benchmark is not None:
            rc, ms = self.benchmark(dx.ptr, L, 1, dspec.ptr, K, M, N, dout.ptr)
            assert rc == 0 and ms > 0.0
        for b in (dx, dspec, dout):
            b.free()

    def check_output_offsets(self, x, h, N):
        """C = 1, K = 64, L = 2^25 + 1000: 2^31 + 64000 output elements; sampled windows of the last two filter rows against np.convolve /
        np.correlate on the matching input slice.  Row K - 1 crosses element 2^31 at n = 2^31 - (K - 1) L: one window straddles it, the
        last ones lie beyond it."""
        sm = self.sm
        (K, M), L = h.shape, x.shape[1]
        W = 3000
        cross = (1 << 31) - (K - 1) * L
        starts = [0, L // 2 + 17, cross - 700, L - 5 * N, L - W]
        assert all(0 <= n0 and n0 + W <= L for n0 in starts) and cross - 700 < cross < cross - 700 + W and (K - 1) * L + L - W >= 1 << 31
        dx, dout = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer(K * L * self.width)
        try:
            for mode in MODES:
                dspec = sm.DeviceBuffer.from_host(self.prepared(h, N, mode))
                assert sm.lib.smfft_memset(dout.ptr, 0xFF, dout.nbytes) == 0
                self.launch(dx.ptr, L, 1, dspec.ptr, K, M, N, dout.ptr, mode)
                assert sm.lib.smfft_synchronize() == 0
                dspec.free()
                for k in (K - 2, K - 1):
                    self.sampled_windows(_Row(dout.ptr + k * L * self.width), x, h[k:k + 1], L, [starts], mode, f"2^31 N={N} {mode} k={k}", W)
        finally:
            dx.free()
            dout.free()

    def check_grid_stride_loop(self, N, mode):
        """M = N - 1 (V = 2 outputs per segment), C = 3, K = 3, U = 10240 F + 1 units per channel (F = 4096 / N per tile): about
        2.5 x 12288 tiles, so every workgroup runs two or three tiles and after its last filter prefetches the first filter's spectrum for
        its next tile.  Tiles straddle channel boundaries for N < 4096 and the last one is partial; the last segment holds one output
        (and, in a real channel, the last pair has no partner).  Every row against fp64."""
        M, C, K = N - 1, 3, 3
        F = 4096 // N
        U = 10240 * F + 1
        L = self.length(U, N, M)
        tiles = self.tiles(L, C, N, M)
        assert self.units(L, N, M) == U and L == 2 * (2 * U - 1 if self.real else U) - 1
        assert 2 * GRID_CAP < tiles < 3 * GRID_CAP and _group_plan(tiles, K) == (3, 1)
        assert F == 1 or (U % F and C * U % F)
        rng = np.random.default_rng(12288 + N + (mode == "correlate"))
        x, h = self.rand(rng, (C, L)), self.rand(rng, (K, M))
        got = self.run(x, h, N, mode)
        _check_rows(got, _reference(x, h, mode == "correlate"), f"grid-stride N={N} {mode}", x, h)

    def check_uneven_groups(self, N, L, K, plan, mode):
        """M = N - 1 on 700 / 450 tiles: filter groups of the rule's size with a shorter last group, and a grid of fewer rows than the
        groups the rule asked for.  Every row equals the K = 1 launch of its filter (the same spectrum) to the bit and is within bounds
        against fp64."""
        M = N - 1
        tiles = self.tiles(L, 1, N, M)
        assert tiles == (700 if K == 7 else 450) and _group_plan(tiles, K) == plan
        asked = min(K, -(-GROUP_TARGET // tiles))
        if K == 7:
            assert asked == plan[1] and K - (plan[1] - 1) * plan[0] == 1       # the last group holds one filter
        else:
            assert asked == 5 and plan[1] == 4                                 # fewer grid rows than groups asked for
        rng = np.random.default_rng(N + K + (mode == "correlate"))
        x, h = self.rand(rng, (1, L)), self.rand(rng, (K, M))
        spectra = self.prepared(h, N, mode)
        got = self.run(x, h, N, mode, spectra=spectra)
        for k in range(K):
            one = self.run(x, h[k:k + 1], N, mode, spectra=spectra[k:k + 1])
            assert np.array_equal(_bits(one[0, 0]), _bits(got[0, k])), (N, K, mode, k)
        _check_rows(got, _reference(x, h, mode == "correlate"), f"groups N={N} K={K} {mode}", x, h)

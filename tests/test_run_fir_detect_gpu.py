"""The detected outputs of the overlap-save FIR filter banks on an MI355X (smfft_fir_power_launch / smfft_fir_peak_launch,
smfft_amd.fir_detect) against fp64 NumPy and against each other: the power of every filter within the complex bank's own per-element
bound (tests/fir_detect_harness.py derives it from ROW_MAX: no new tolerance); the peak launch equal to np.max / np.argmax of the
library's own power rows to the bit, and within the bound of the fp64 maximum; exact probes (identical filters, power-of-two filters, a
NaN sample, a NaN tap); the filter groups; the grid-stride loop; guarded buffers at interior bases; 64-bit offsets; a caller's stream,
the benchmark form and the host round trips.

Every run goes into outputs prefilled with 0xFF and followed by a guard of 4096 elements of 0x5A that must stay untouched, and every
index must lie in [0, K).

The file's name makes it collect behind the older GPU test files, as tests/test_real_fir_gpu.py's does, so that every older test keeps
its place in a run of the suite."""
import ctypes

import numpy as np
import pytest

from tests.fir_detect_harness import MODES, ROW_MAX, Detect, _rand, _reference, bits, case, power64

import fir_plan_model as fm  # noqa: E402  (tools/ is on the path through the harness)

pytestmark = pytest.mark.gpu

SIZES = [256, 512, 1024, 2048, 4096]
ENDS = [256, 4096]


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def fd():
    from smfft_amd import fir_detect
    fir_detect.lib()
    return fir_detect


@pytest.fixture(scope="module")
def det(sm, fd):
    return Detect(sm, fd)


def _taps(N):
    return (1, 17, N // 4 + 1, N - 1)


# ---- 1 - 3: fp64 and the library's own power ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_power_against_fp64(det, N, mode):
    """every N, both modes, M in {1, 17, N/4 + 1, N - 1}, C = 2, K = 3, L = 3 V + 5: per element
    |p - p64| <= 2 |y64| E + E^2 + 2^-22 p64, E = ROW_MAX max(max |y64 row|, ||h_k|| max |x_c|)"""
    for M in _taps(N):
        x, h, y64 = case(N, mode, M, 3)
        got = det.run(x, h, N, mode, which=("power",))["power"]
        det.check_power(got, y64, x, h, f"N={N} {mode} M={M}")


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_peak_equals_the_librarys_own_power(det, N, mode):
    """the same cases with K = 1 and K = 5: peak's bits equal np.max(power, axis=1)'s and index == np.argmax(power, axis=1) everywhere"""
    for M in _taps(N):
        for K in (1, 5):
            x, h, _ = case(N, mode, M, K)
            det.check_peak_is_own_power(det.run(x, h, N, mode), f"N={N} {mode} M={M} K={K}")


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_peak_against_fp64(det, N, mode):
    """the cases of the two tests above (K = 1, 3, 5), none left out: the peak within the largest of the K row bounds of the fp64
    maximum, and the fp64 power of the chosen filter within twice that bound of the fp64 maximum"""
    for M in _taps(N):
        for K in (1, 3, 5):
            x, h, y64 = case(N, mode, M, K)
            out = det.run(x, h, N, mode, which=("peak",))
            det.check_peak(out["peak"], out["index"], y64, x, h, f"N={N} {mode} M={M} K={K}")


# ---- 4: exact probes --------------------------------------------------------------------------------------------------------------
def _probe_shape(N):
    M = N // 4 + 1
    return M, 3 * (N - M + 1) + 5


@pytest.mark.parametrize("N", ENDS)
@pytest.mark.parametrize("mode", MODES)
def test_probe_identical_filters(det, N, mode):
    """filters 3 and 7 of K = 9 identical: their power rows are bit-identical, and the index is never 7 (the lowest filter wins a tie)"""
    rng = np.random.default_rng(40 + N)
    M, L = _probe_shape(N)
    x, h = _rand(rng, (2, L)), _rand(rng, (9, M))
    h[7] = h[3]
    out = det.run(x, h, N, mode)
    assert np.array_equal(bits(out["power"][:, 3]), bits(out["power"][:, 7]))
    assert not np.any(out["index"] == 7) and np.any(out["index"] == 3)
    det.check_peak_is_own_power(out, f"identical filters N={N} {mode}")


@pytest.mark.parametrize("N", ENDS)
@pytest.mark.parametrize("mode", MODES)
def test_probe_power_of_two_filters(det, N, mode):
    """h_k = 2^s_k h_0, s a permutation of -3 ... 3 with s_0 = 0: the power rows are exactly 4^s_k times row 0, and the index is
    argmax s wherever row 0 is non-zero and 0 elsewhere (channel 1 is all zeros: every power there is +0, and the first filter keeps a
    tie)"""
    rng = np.random.default_rng(41 + N)
    M, L = _probe_shape(N)
    s = np.array([0, -2, 3, -3, 1, 2, -1])
    x, h0 = _rand(rng, (2, L)), _rand(rng, (1, M))
    x[1] = 0
    h = np.ldexp(h0.real, s[:, None]).astype(np.float32) + 1j * np.ldexp(h0.imag, s[:, None]).astype(np.float32)
    h = h.astype(np.complex64)
    assert np.array_equal(h[0], h0[0])
    out = det.run(x, h, N, mode)
    row0 = out["power"][:, 0]
    for k in range(len(s)):
        assert np.array_equal(bits(out["power"][:, k]), bits(np.ldexp(row0, 2 * s[k]).astype(np.float32))), (N, mode, k)
    assert np.array_equal(out["index"], np.where(row0 != 0, int(np.argmax(s)), 0)), (N, mode)
    assert np.all(row0[1] == 0) and np.all(out["index"][1] == 0) and np.all(out["peak"][1] == 0)
    assert np.array_equal(bits(out["peak"]), bits(np.ldexp(row0, 2 * int(s.max())).astype(np.float32)))


def _segments_reading(w, n):
    return [s for s in range(w.segments()) if w.load_start(s) <= n < w.load_start(s) + w.N]


@pytest.mark.parametrize("N", ENDS)
@pytest.mark.parametrize("mode", MODES)
def test_probe_nan_sample(det, N, mode):
    """one NaN sample in channel 1 of 2: exactly the outputs of the segments that read it are NaN in every power row of that channel,
    and NaN with index 0 in the peak; all others are bit-identical to the clean run.  The sample sits in the overlap of two segments,
    and where one segment alone reads it (the last sample; for a correlation, whose segments look ahead, the first)"""
    corr = mode == "correlate"
    rng = np.random.default_rng(42 + N + corr)
    M, L = _probe_shape(N)
    K, V = 4, N - M + 1
    w = fm.Window(L, N, M, corr)
    x, h = _rand(rng, (2, L)), _rand(rng, (K, M))
    spectra = det.prepared(h, N, mode)
    clean = det.run(x, h, N, mode, spectra=spectra)
    overlap = 2 * V if corr else 2 * V - 1                 # the look-ahead of segment 1 / the history of segment 2
    alone = 0 if corr else L - 1                           # read by the first / the last segment alone
    assert w.segments() == 4 and _segments_reading(w, overlap) == [1, 2] and _segments_reading(w, alone) == [0 if corr else 3]
    for n in (overlap, alone):
        foot = np.zeros(L, bool)
        for seg in _segments_reading(w, n):
            b, e = w.store_window(seg)
            foot[w.output_index(seg, b):w.output_index(seg, e)] = True
        bad = x.copy()
        bad[1, n] = np.nan
        got = det.run(bad, h, N, mode, spectra=spectra, finite=False)
        for k in range(K):
            assert np.array_equal(np.isnan(got["power"][1, k]), foot), (N, mode, n, k)
            assert np.array_equal(bits(got["power"][1, k][~foot]), bits(clean["power"][1, k][~foot])), (N, mode, n, k)
        assert np.array_equal(np.isnan(got["peak"][1]), foot) and np.all(got["index"][1][foot] == 0), (N, mode, n)
        assert np.array_equal(bits(got["peak"][1][~foot]), bits(clean["peak"][1][~foot])), (N, mode, n)
        assert np.array_equal(got["index"][1][~foot], clean["index"][1][~foot]), (N, mode, n)
        for name in ("power", "peak", "index"):
            assert np.array_equal(bits(got[name][0]), bits(clean[name][0])), (N, mode, n, name)


@pytest.mark.parametrize("N", ENDS)
@pytest.mark.parametrize("mode", MODES)
def test_probe_nan_tap(det, N, mode):
    """a NaN tap in filter 2 of 4: power row 2 is all NaN, the other rows equal the clean run to the bit, and the peak is NaN with
    index 2 everywhere"""
    rng = np.random.default_rng(43 + N)
    M, L = _probe_shape(N)
    x, h = _rand(rng, (2, L)), _rand(rng, (4, M))
    bad = h.copy()
    bad[2, M // 2] = np.nan
    clean = det.run(x, h, N, mode)
    got = det.run(x, bad, N, mode, finite=False)
    assert np.isnan(got["power"][:, 2]).all(), (N, mode)
    assert np.array_equal(bits(got["power"][:, [0, 1, 3]]), bits(clean["power"][:, [0, 1, 3]])), (N, mode)
    assert np.isnan(got["peak"]).all() and np.all(got["index"] == 2), (N, mode)


# ---- 5, 6: the filter groups and the grid-stride loop ------------------------------------------------------------------------------
def test_filter_groups(det, sm, fd):
    """K = 200 on one short channel at N = 1024, M = 257 (20 workgroup tiles: the power launch splits the filters into 100 groups of
    2): every power row equals its K = 1 launch to the bit; the peak launch on the same input, one group of 200, equals the max /
    argmax of those rows"""
    N, M, K = 1024, 257, 200
    L = 20 * (4096 // N) * (N - M + 1) - 7
    rng = np.random.default_rng(N)
    x, h = _rand(rng, (1, L)), _rand(rng, (K, M))
    for mode in MODES:
        spectra = det.prepared(h, N, mode)
        out = det.run(x, h, N, mode, spectra=spectra)
        dx, dspec, d1 = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer.from_host(spectra), sm.DeviceBuffer(L * 4)
        for k in range(K):
            fd.power_launch(dx.ptr, L, 1, dspec.ptr + k * N * 8, 1, M, N, d1.ptr, mode)
            assert sm.lib.smfft_synchronize() == 0
            assert np.array_equal(bits(d1.to_host(np.float32, (L,))), bits(out["power"][0, k])), (mode, k)
        for b in (dx, dspec, d1):
            b.free()
        det.check_peak_is_own_power(out, f"K={K} {mode}")
        det.check_power(out["power"][:, ::37], _reference(x, h[::37], mode == "correlate"), x, h[::37], f"K={K} {mode}")


@pytest.mark.parametrize("N", ENDS)
@pytest.mark.parametrize("mode", MODES)
def test_grid_stride_loop(det, N, mode):
    """the shape of tests/fir_gpu_harness.py check_grid_stride_loop: M = N - 1 (V = 2), C = 3, K = 3, 10240 F + 1 segments per channel
    (F = 4096 / N per tile): about 2.5 x 12288 tiles, so every workgroup runs two or three tiles and after its last filter prefetches
    the first filter's spectrum for its next tile.  Power against the bound; peak against power to the bit"""
    M, C, K = N - 1, 3, 3
    F = 4096 // N
    S = 10240 * F + 1
    L = (S - 1) * 2 + 1
    tiles = -(-S * C // F)
    assert fm.Window(L, N, M, False).segments() == S and 2 * 12288 < tiles < 3 * 12288
    rng = np.random.default_rng(12288 + N + (mode == "correlate"))
    x, h = _rand(rng, (C, L)), _rand(rng, (K, M))
    out = det.run(x, h, N, mode)
    det.check_power(out["power"], _reference(x, h, mode == "correlate"), x, h, f"grid-stride N={N} {mode}")
    det.check_peak_is_own_power(out, f"grid-stride N={N} {mode}")


# ---- 7: bounds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", ENDS)
@pytest.mark.parametrize("mode", MODES)
def test_bounds(det, N, mode):
    """both launches with the output and index base pointers 1 and 3 elements inside their allocations (4-byte aligned, not 8), the
    signal ending where its allocation ends, L in {1, V, V + 1}: nothing in front of or behind the outputs changes, every output is
    written, and the results equal those at an aligned base to the bit and pass the fp64 bound"""
    rng = np.random.default_rng(70 + N + (mode == "correlate"))
    for M in (N // 4 + 1, N - 1):
        V = N - M + 1
        for L in (1, V, V + 1):
            x, h = _rand(rng, (2, L)), _rand(rng, (3, M))
            spectra = det.prepared(h, N, mode)
            base = det.run(x, h, N, mode, spectra=spectra, exact_signal=True)
            what = f"N={N} {mode} M={M} L={L}"
            det.check_power(base["power"], _reference(x, h, mode == "correlate"), x, h, what)
            det.check_peak_is_own_power(base, what)
            for front in (1, 3):
                got = det.run(x, h, N, mode, spectra=spectra, front=front, exact_signal=True)
                for name in ("power", "peak", "index"):
                    assert np.array_equal(bits(got[name]), bits(base[name])), f"{what} front={front}: {name} depends on placement"


# ---- 8: 64-bit offsets ---------------------------------------------------------------------------------------------------------------
def test_power_offsets_beyond_two_to_the_31(det, sm, fd):
    """N = 1024, C = 1, K = 64, L = 2^25 + 1000: 2^31 + 64000 power floats.  Sampled windows of the last two rows against
    |np.convolve|^2 on the matching input slice, with test 1's bound on the window.  Row K - 1 crosses element 2^31 at
    n = 2^31 - (K - 1) L: one window straddles it, the last ones lie beyond it.

    The peak launch is not run at this size: its outputs hold C L elements, their offsets c L + n are formed in the same 64-bit
    expression as the power launch's (c K + k) L + n, and reaching 2^31 there takes a signal of 16 GiB."""
    N, M, K, L, W = 1024, 257, 64, (1 << 25) + 1000, 3000
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((1, L), dtype=np.float32) + 1j * rng.standard_normal((1, L), dtype=np.float32)).astype(np.complex64)
    h = _rand(rng, (K, M))
    cross = (1 << 31) - (K - 1) * L
    starts = [0, L // 2 + 17, cross - 700, L - 5 * N, L - W]
    assert all(0 <= n0 and n0 + W <= L for n0 in starts) and cross - 700 < cross < cross - 700 + W and (K - 1) * L + L - W >= 1 << 31
    dx, dspec = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer.from_host(det.prepared(h, N, "convolve"))
    dout, pout = det.guarded(K * L)
    try:
        fd.power_launch(dx.ptr, L, 1, dspec.ptr, K, M, N, pout, "convolve")
        assert sm.lib.smfft_synchronize() == 0
        guard = np.empty(4096, np.uint32)
        assert sm.lib.smfft_memcpy_d2h(guard.ctypes.data, pout + 4 * K * L, guard.nbytes) == 0
        assert np.all(guard == 0x5A5A5A5A), "the kernel wrote past its output"
        for k in (K - 2, K - 1):
            hk = h[k].astype(np.complex128)
            for n0 in starts:
                got = np.empty(W, np.float32)
                assert sm.lib.smfft_memcpy_d2h(got.ctypes.data, pout + 4 * (k * L + n0), got.nbytes) == 0
                lo = max(0, n0 - (M - 1))
                seg = x[0, lo:n0 + W].astype(np.complex128)
                y64 = np.convolve(seg, hk)[n0 - lo:n0 - lo + W]
                assert np.all(np.isfinite(got)), (k, n0)
                det.check_power(got[None, None], y64[None, None], seg[None], h[k:k + 1], f"2^31 k={k} n0={n0}")
    finally:
        for b in (dx, dspec, dout):
            b.free()


# ---- 9: entry forms ----------------------------------------------------------------------------------------------------------------
def test_caller_stream(det, fd):
    """both launches on a stream from hipStreamCreate, then hipStreamSynchronize"""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value
    N, M, C, K, L = 1024, 257, 2, 9, 50000
    rng = np.random.default_rng(11)
    x, h = _rand(rng, (C, L)), _rand(rng, (K, M))
    for mode in MODES:
        def launch(name, dx, dspec, outputs):
            getattr(fd, name + "_launch")(dx, L, C, dspec, K, M, N, *outputs, mode=mode, stream=stream.value)
            assert hip.hipStreamSynchronize(stream) == 0
        out = det.run(x, h, N, mode, launch=launch)
        det.check_power(out["power"], _reference(x, h, mode == "correlate"), x, h, f"stream {mode}")
        det.check_peak_is_own_power(out, f"stream {mode}")
    assert hip.hipStreamDestroy(stream) == 0


def test_benchmark_form_adds_to_the_timer(det, fd):
    """the library's *_benchmark functions add their milliseconds to a non-zero total and fill the outputs; so do the mirror's"""
    N, M, C, K, L = 512, 100, 1, 3, 20000
    rng = np.random.default_rng(12)
    x, h = _rand(rng, (C, L)), _rand(rng, (K, M))
    total = ctypes.c_double(1.0)
    seen = []

    def launch(name, dx, dspec, outputs):
        before = total.value
        assert getattr(fd.lib(), f"smfft_fir_{name}_benchmark")(dx, L, C, dspec, K, M, N, 0, *outputs, ctypes.byref(total)) == 0
        assert total.value > before >= 1.0
        seen.append(name)
    out = det.run(x, h, N, "convolve", launch=launch)
    assert seen == ["power", "peak"]
    det.check_power(out["power"], _reference(x, h, False), x, h, "benchmark form")
    det.check_peak_is_own_power(out, "benchmark form")

    def mirror(name, dx, dspec, outputs):
        rc, ms = getattr(fd, name + "_benchmark")(dx, L, C, dspec, K, M, N, *outputs)
        assert rc == 0 and ms > 0.0
    again = det.run(x, h, N, "convolve", launch=mirror)
    for name in ("power", "peak", "index"):
        assert np.array_equal(bits(again[name]), bits(out[name])), name


def test_host_round_trips(det, fd):
    """fir_detect.power / peak: 1-D and (C, L) inputs, complex128 input, the default transform length (the 4 M rule), the (C, K, L)
    float32 and (C, L) float32 / int32 results, equal to the device-pointer launches to the bit"""
    rng = np.random.default_rng(7)
    x = rng.standard_normal(5000) + 1j * rng.standard_normal(5000)
    h = rng.standard_normal(65) + 1j * rng.standard_normal(65)
    x32, h32 = x.astype(np.complex64)[None], h.astype(np.complex64)[None]
    for mode in MODES:
        p = fd.power(x, h, mode)
        best, index = fd.peak(x, h, mode)
        assert p.shape == (1, 1, 5000) and p.dtype == np.float32
        assert best.shape == index.shape == (1, 5000) and best.dtype == np.float32 and index.dtype == np.int32
        det.check_power(p, _reference(x32, h32, mode == "correlate"), x32, h32, f"power() {mode}")
        assert np.array_equal(bits(best), bits(p[:, 0])) and not index.any()
    x2, h2 = _rand(rng, (2, 3000)), _rand(rng, (3, 33))
    p = fd.power(x2, h2, fft_size=1024)
    best, index = fd.peak(x2, h2, fft_size=1024)
    want = det.run(x2, h2, 1024, "convolve")
    assert p.shape == (2, 3, 3000) and np.array_equal(bits(p), bits(want["power"]))
    assert np.array_equal(bits(best), bits(want["peak"])) and np.array_equal(index, want["index"])
    assert ROW_MAX == 5e-6 and power64(np.array([3 + 4j])) == 25.0

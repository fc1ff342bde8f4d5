"""The overlap-save FIR filter banks on an MI355X (smfft_fir_prepare / smfft_fir_launch, smfft_amd.fir*) against fp64 NumPy: both modes at
every transform length over a grid of taps, channels, filters and signal lengths; the filter-group split, uneven groups included; the
grid-stride loop past the grid cap; the prepared spectra; a caller's stream; 64-bit output offsets.

Tolerances per (channel, filter) row: relL2 <= 1e-6 and max|err| / max|ref| <= 5e-6 -- two fp32 transforms and a product, at the
library's per-FFT bounds (5e-7 / 1e-6, oracle/np_reference.py) each.  The rounding error of an FFT convolution is spread over the
whole segment: per output it scales with ||h_k||_2 ||x_c||_2, not with |y[n]|.  Outputs that are partial sums (the first M - 1 of a
convolution, the last M - 1 of a correlation) are small against that scale, and a row made of nothing else (L < M) can miss the bounds
by an order of magnitude while every transform is as accurate as anywhere else (N = 256, M = 255, L = 2: relL2 1.1e-6 against the
row's own norm).  So the denominators are max(||y_row||, ||h_k|| ||x_c||) and max(max|y_row|, ||h_k|| max|x_c|): for rows of full
M-term sums these are the row's own norm and maximum (to within sampling), for rows of partial sums the scale the transforms carry."""
import ctypes

import numpy as np
import pytest

from oracle.np_reference import MAX_ABS_TOL, REL_L2_TOL
from tests.fir_gpu_harness import GUARD, MODES, _check_rows, _rand, _reference, _sampled_windows      # (puts tools/ on the path)

import fir_plan_model as fm  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [256, 512, 1024, 2048, 4096]


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    smfft_amd.FFT_init()
    return smfft_amd


def _run(sm, x, h, N, mode, spectra=None):
    """prepare + launch through the device-pointer API into an output followed by a guard region; returns the (C, K, L) result
    after checking that the guard is untouched and no NaN of the prefill is left"""
    C, L = x.shape
    K, M = h.shape
    dx, dh = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer.from_host(h)
    if spectra is None:
        dspec = sm.DeviceBuffer(K * N * 8)
        sm.fir_prepare(dh.ptr, dspec.ptr, M, K, N, mode)
    else:
        dspec = sm.DeviceBuffer.from_host(spectra)
    total = C * K * L
    dout = sm.DeviceBuffer((total + GUARD) * 8)
    assert sm.lib.smfft_memset(dout.ptr, 0xFF, total * 8) == 0
    assert sm.lib.smfft_memset(dout.ptr + total * 8, 0x5A, GUARD * 8) == 0
    sm.fir_launch(dx.ptr, L, C, dspec.ptr, K, M, N, dout.ptr, mode)
    assert sm.lib.smfft_synchronize() == 0
    raw = dout.to_host(np.uint8, ((total + GUARD) * 8,))
    assert np.all(raw[total * 8:] == 0x5A), "the kernel wrote past its output"
    out = raw[:total * 8].view(np.complex64).reshape(C, K, L)
    assert np.all(np.isfinite(out.view(np.float32))), "outputs left unwritten"
    for b in (dx, dh, dspec, dout):
        b.free()
    return out


def test_reference_is_numpys_definition():
    rng = np.random.default_rng(1)
    x, h = _rand(rng, (2, 300)), _rand(rng, (3, 17))
    for corr in (False, True):
        want = fm.direct(x, h, corr)
        assert np.max(np.abs(_reference(x, h, corr) - want)) <= 1e-12 * np.max(np.abs(want))


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_filter_bank_matches_numpy(sm, N, mode):
    rng = np.random.default_rng(N + (mode == "correlate"))
    F = 4096 // N                                    # segments per workgroup tile
    for M in (1, 17, N // 4 + 1, N - 1):
        V = N - M + 1
        # L < M; one segment; F + 1 segments per channel (3 channels: tiles partly empty and straddling channel boundaries)
        lengths = [max(1, M // 2) if M > 1 else 1, V, (F + 1) * V - 3]
        for L in lengths:
            for C, K in ((1, 1), (3, 5), (1, 64), (3, 64)):
                x, h = _rand(rng, (C, L)), _rand(rng, (K, M))
                got = _run(sm, x, h, N, mode)
                _check_rows(got, _reference(x, h, mode == "correlate"), f"N={N} {mode} M={M} L={L} C={C} K={K}", x, h)


def test_host_convenience(sm):
    """fir(): 1-D and real inputs, the default transform length, the (C, K, L) result"""
    rng = np.random.default_rng(7)
    x = rng.standard_normal(5000).astype(np.float32)
    h = _rand(rng, (65,))
    for mode in MODES:
        got = sm.fir(x, h, mode)
        assert got.shape == (1, 1, 5000) and got.dtype == np.complex64
        _check_rows(got, _reference(x[None].astype(np.complex64), h[None], mode == "correlate"), f"fir() {mode}", x[None], h[None])
    got = sm.fir(_rand(rng, (2, 3000)), _rand(rng, (3, 33)), fft_size=1024)
    assert got.shape == (2, 3, 3000)


@pytest.mark.parametrize("N,M", [(256, 65), (1024, 257), (4096, 1025)])
def test_filter_group_split_is_bit_exact(sm, N, M):
    """K = 200 on a signal of 20 workgroup tiles: the launch splits the filters into 100 groups of 2 (fir_filter_group_size); every
    row equals the K = 1 launch of its filter to the bit"""
    rng = np.random.default_rng(N)
    V, F, K = N - M + 1, 4096 // N, 200
    L = 20 * F * V - 7
    x, h = _rand(rng, (1, L)), _rand(rng, (K, M))
    for mode in MODES:
        dx, dh = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer.from_host(h)
        dspec, dout, d1 = sm.DeviceBuffer(K * N * 8), sm.DeviceBuffer(K * L * 8), sm.DeviceBuffer(L * 8)
        sm.fir_prepare(dh.ptr, dspec.ptr, M, K, N, mode)
        sm.fir_launch(dx.ptr, L, 1, dspec.ptr, K, M, N, dout.ptr, mode)
        assert sm.lib.smfft_synchronize() == 0
        all_rows = dout.to_host(np.complex64, (K, L))
        for k in range(K):
            sm.fir_launch(dx.ptr, L, 1, dspec.ptr + k * N * 8, 1, M, N, d1.ptr, mode)
            assert sm.lib.smfft_synchronize() == 0
            one = d1.to_host(np.complex64, (L,))
            assert np.array_equal(one.view(np.uint32), all_rows[k].view(np.uint32)), (mode, k)
        _check_rows(all_rows[None, ::37], _reference(x, h[::37], mode == "correlate"), f"K=200 N={N} {mode}", x, h[::37])
        for b in (dx, dh, dspec, dout, d1):
            b.free()


@pytest.mark.parametrize("N", SIZES)
def test_prepared_spectra(sm, N):
    """smfft_fir_prepare = fft(pad(g)) / N within the per-FFT tolerances; a launch with NumPy-prepared spectra gives the library's result"""
    rng = np.random.default_rng(3 * N)
    K = 7
    for mode in MODES:
        for M in (1, 17, N // 4 + 1, N - 1):
            h = _rand(rng, (K, M))
            dh, dspec = sm.DeviceBuffer.from_host(h), sm.DeviceBuffer(K * N * 8)
            sm.fir_prepare(dh.ptr, dspec.ptr, M, K, N, mode)
            assert sm.lib.smfft_synchronize() == 0
            got = dspec.to_host(np.complex64, (K, N))
            want = fm.spectra(h, N, mode == "correlate")
            for k in range(K):
                d = got[k] - want[k]
                l2 = np.linalg.norm(d) / np.linalg.norm(want[k])
                mx = np.max(np.abs(d)) / np.max(np.abs(want[k]))
                assert l2 <= REL_L2_TOL and mx <= MAX_ABS_TOL, (mode, M, k, l2, mx)
            dh.free()
            dspec.free()
            x = _rand(rng, (2, 3 * (N - M + 1) + 5))
            lib_out = _run(sm, x, h, N, mode)
            np_out = _run(sm, x, h, N, mode, spectra=want.astype(np.complex64))
            want_y = _reference(x, h, mode == "correlate")
            _check_rows(np_out, want_y, f"NumPy spectra N={N} {mode} M={M}", x, h)
            _check_rows(lib_out, np_out.astype(np.complex128), f"library vs NumPy spectra N={N} {mode} M={M}", x, h)


def test_caller_stream(sm):
    """prepare and launch on a stream from hipStreamCreate, then hipStreamSynchronize"""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value
    rng = np.random.default_rng(11)
    N, M, C, K, L = 1024, 257, 2, 9, 50000
    x, h = _rand(rng, (C, L)), _rand(rng, (K, M))
    for mode in MODES:
        dx, dh = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer.from_host(h)
        dspec, dout = sm.DeviceBuffer(K * N * 8), sm.DeviceBuffer(C * K * L * 8)
        assert sm.lib.smfft_memset(dout.ptr, 0xFF, dout.nbytes) == 0
        assert sm.lib.smfft_synchronize() == 0
        sm.fir_prepare(dh.ptr, dspec.ptr, M, K, N, mode, stream=stream.value)
        sm.fir_launch(dx.ptr, L, C, dspec.ptr, K, M, N, dout.ptr, mode, stream=stream.value)
        assert hip.hipStreamSynchronize(stream) == 0
        _check_rows(dout.to_host(np.complex64, (C, K, L)), _reference(x, h, mode == "correlate"), f"stream {mode}", x, h)
        for b in (dx, dh, dspec, dout):
            b.free()
    assert hip.hipStreamDestroy(stream) == 0


def test_benchmark_form(sm):
    rng = np.random.default_rng(12)
    N, M, K, L = 512, 100, 3, 20000
    x, h = _rand(rng, (1, L)), _rand(rng, (K, M))
    dx, dh = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer.from_host(h)
    dspec, dout = sm.DeviceBuffer(K * N * 8), sm.DeviceBuffer(K * L * 8)
    sm.fir_prepare(dh.ptr, dspec.ptr, M, K, N)
    t = ctypes.c_double(1.0)
    assert sm.lib.smfft_fir_benchmark(dx.ptr, L, 1, dspec.ptr, K, M, N, 0, dout.ptr, ctypes.byref(t)) == 0
    assert t.value > 1.0
    _check_rows(dout.to_host(np.complex64, (1, K, L)), _reference(x, h, False), "benchmark form", x, h)
    for b in (dx, dh, dspec, dout):
        b.free()


def test_output_offsets_beyond_two_to_the_31(sm):
    """C = 1, K = 64, L = 2^25 + 1000: 2.15e9 output elements (16 GiB); sampled windows of the last filter rows against np.convolve /
    np.correlate on the matching input slice"""
    N, M, K, L = 1024, 257, 64, (1 << 25) + 1000
    rng = np.random.default_rng(5)
    x = _rand(rng, (1, L))
    h = _rand(rng, (K, M))
    dx, dh = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer.from_host(h)
    dspec, dout = sm.DeviceBuffer(K * N * 8), sm.DeviceBuffer(K * L * 8)
    W = 3000
    # row K - 1 crosses element 2^31 (byte offset 16 GiB) at n = 2^31 - (K - 1) L: one window straddles it, the last ones lie beyond it
    cross = (1 << 31) - (K - 1) * L
    starts = [0, L // 2 + 17, cross - 700, L - 5 * N, L - W]
    assert all(0 <= n0 and n0 + W <= L for n0 in starts) and (K - 1) * L + L - W >= 1 << 31
    for mode in MODES:
        corr = mode == "correlate"
        sm.fir_prepare(dh.ptr, dspec.ptr, M, K, N, mode)
        sm.fir_launch(dx.ptr, L, 1, dspec.ptr, K, M, N, dout.ptr, mode)
        assert sm.lib.smfft_synchronize() == 0
        for k in (K - 2, K - 1):
            for n0 in starts:
                got = np.empty(W, np.complex64)
                assert sm.lib.smfft_memcpy_d2h(got.ctypes.data, dout.ptr + (k * L + n0) * 8, W * 8) == 0
                hk = h[k].astype(np.complex128)
                if corr:
                    seg = np.r_[x[0, n0:n0 + W + M - 1].astype(np.complex128), np.zeros(max(0, n0 + W + M - 1 - L))]
                    want = np.correlate(seg, hk, "valid")
                else:
                    lo = max(0, n0 - (M - 1))
                    seg = x[0, lo:n0 + W].astype(np.complex128)
                    want = np.convolve(seg, hk)[n0 - lo:n0 - lo + W]
                _check_rows(got[None, None], want[None, None], f"{mode} k={k} n0={n0}", seg[None], hk[None])
    for b in (dx, dh, dspec, dout):
        b.free()


# ---- the grid-stride loop and the filter groups ------------------------------------------------------------------------------
GRID_CAP = 12288               # smfft_fir.hip kFirGridCap: workgroups along the segment tiles; more tiles are grid-strided
GROUP_TARGET = 2048            # smfft_fir.hip kFirTargetWorkgroups: the filter-group rule's target


def _tiles(L, C, N, M):
    return -(-fm.Window(L, N, M, False).segments() * C // (4096 // N))


def _group_plan(tiles, K):
    """(group size, grid rows) of a launch: the rule of smfft_fir.hpp fir_filter_group_size, restated"""
    groups = max(1, min(K, -(-GROUP_TARGET // tiles)))
    size = -(-K // groups)
    return size, -(-K // size)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_grid_stride_loop_with_wrapped_prefetch(sm, N, mode):
    """M = N - 1 (V = 2 outputs per segment), C = 3, K = 3: about 2.5 x 12288 tiles, so every workgroup runs two or three tiles and
    after its last filter prefetches the first filter's spectrum for its next tile.  S = 10240 F + 1 segments per channel (F = 4096 / N
    per tile): tiles straddle channel boundaries for N < 4096 and the last one is partial; L = 2 S - 1 leaves the last segment one
    output.  Every row against fp64."""
    M, C, K = N - 1, 3, 3
    F = 4096 // N
    S = 10240 * F + 1
    L = 2 * S - 1
    tiles = _tiles(L, C, N, M)
    assert 2 * GRID_CAP < tiles < 3 * GRID_CAP and _group_plan(tiles, K) == (3, 1)
    assert F == 1 or (S % F and C * S % F)
    rng = np.random.default_rng(12288 + N + (mode == "correlate"))
    x, h = _rand(rng, (C, L)), _rand(rng, (K, M))
    got = _run(sm, x, h, N, mode)
    _check_rows(got, _reference(x, h, mode == "correlate"), f"grid-stride N={N} {mode}", x, h)


@pytest.mark.parametrize("mode", MODES)
def test_grid_stride_loop_at_a_realistic_shape(sm, mode):
    """N = 1024, M = 257, C = 3 channels of L = 16e6 samples, K = 2: 15,626 tiles, past the grid cap.  Sampled windows against
    np.convolve / np.correlate: the first and last of every (channel, filter) row (their segments' tiles straddle two channels), one in
    the middle, and the one where the grid-stride loop's second pass starts (tile 12288)."""
    N, M, C, K, L = 1024, 257, 3, 2, 16_000_000
    V, F = N - M + 1, 4096 // N
    S = -(-L // V)
    tiles = _tiles(L, C, N, M)
    assert tiles > GRID_CAP and S % F and _group_plan(tiles, K) == (2, 1)
    rng = np.random.default_rng(16)
    x = rng.standard_normal((C, 2 * L), dtype=np.float32).view(np.complex64)
    h = _rand(rng, (K, M))
    W = 3000
    starts = [[0, L // 2 + 11, L - W] for _ in range(C)]
    c2, s2 = divmod(GRID_CAP * F, S)                  # the first segment of tile 12288
    starts[c2].append(max(0, s2 * V - W // 2))
    dx, dh = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer.from_host(h)
    dspec, dout = sm.DeviceBuffer(K * N * 8), sm.DeviceBuffer((C * K * L + GUARD) * 8)
    try:
        assert sm.lib.smfft_memset(dout.ptr + C * K * L * 8, 0x5A, GUARD * 8) == 0
        sm.fir_prepare(dh.ptr, dspec.ptr, M, K, N, mode)
        sm.fir_launch(dx.ptr, L, C, dspec.ptr, K, M, N, dout.ptr, mode)
        assert sm.lib.smfft_synchronize() == 0
        guard = np.empty(GUARD * 8, np.uint8)
        assert sm.lib.smfft_memcpy_d2h(guard.ctypes.data, dout.ptr + C * K * L * 8, GUARD * 8) == 0
        assert np.all(guard == 0x5A), "the kernel wrote past its output"
        _sampled_windows(sm, dout, x, h, L, starts, mode, f"L=16e6 {mode}", W)
    finally:
        for b in (dx, dh, dspec, dout):
            b.free()


@pytest.mark.parametrize("N,L,K,plan", [
    (4096, 2 * 700 - 1, 7, (3, 3)),      # 3 groups of 3 filters asked and launched; the last holds one
    (4096, 2 * 450 - 1, 12, (3, 4)),     # 5 groups asked, group size 3: 4 grid rows
    (256, 2 * (699 * 16 + 5) - 1, 7, (3, 3)),
    (256, 2 * (449 * 16 + 7) - 1, 12, (3, 4)),
])
@pytest.mark.parametrize("mode", MODES)
def test_uneven_filter_groups(sm, N, L, K, plan, mode):
    """M = N - 1 on 700 / 450 tiles: filter groups of the rule's size with a shorter last group, and a grid of fewer rows than the
    groups the rule asked for.  Every row equals the K = 1 launch of its filter (the same spectrum) to the bit and is within bounds
    against fp64."""
    M = N - 1
    tiles = _tiles(L, 1, N, M)
    assert tiles == (700 if K == 7 else 450) and _group_plan(tiles, K) == plan
    asked = min(K, -(-GROUP_TARGET // tiles))
    if K == 7:
        assert asked == plan[1] and K - (plan[1] - 1) * plan[0] == 1       # the last group holds one filter
    else:
        assert asked == 5 and plan[1] == 4                                 # fewer grid rows than groups asked for
    rng = np.random.default_rng(N + K + (mode == "correlate"))
    x, h = _rand(rng, (1, L)), _rand(rng, (K, M))
    dh, dspec = sm.DeviceBuffer.from_host(h), sm.DeviceBuffer(K * N * 8)
    sm.fir_prepare(dh.ptr, dspec.ptr, M, K, N, mode)
    assert sm.lib.smfft_synchronize() == 0
    spectra = dspec.to_host(np.complex64, (K, N))
    dh.free()
    dspec.free()
    got = _run(sm, x, h, N, mode, spectra=spectra)
    for k in range(K):
        one = _run(sm, x, h[k:k + 1], N, mode, spectra=spectra[k:k + 1])
        assert np.array_equal(one[0, 0].view(np.uint32), got[0, k].view(np.uint32)), (N, K, mode, k)
    _check_rows(got, _reference(x, h, mode == "correlate"), f"groups N={N} K={K} {mode}", x, h)

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
import numpy as np
import pytest

from tests.fir_gpu_harness import GRID_CAP, GUARD, MODES, Bank, _check_rows, _group_plan, _rand, _reference      # (puts tools/ on the path)

import fir_plan_model as fm  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [256, 512, 1024, 2048, 4096]


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def bank(sm):
    return Bank.complex(sm)


def test_reference_is_numpys_definition():
    rng = np.random.default_rng(1)
    x, h = _rand(rng, (2, 300)), _rand(rng, (3, 17))
    for corr in (False, True):
        want = fm.direct(x, h, corr)
        assert np.max(np.abs(_reference(x, h, corr) - want)) <= 1e-12 * np.max(np.abs(want))


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_filter_bank_matches_numpy(bank, N, mode):
    rng = np.random.default_rng(N + (mode == "correlate"))
    F = 4096 // N                                    # segments per workgroup tile
    for M in (1, 17, N // 4 + 1, N - 1):
        V = N - M + 1
        # L < M; one segment; F + 1 segments per channel (3 channels: tiles partly empty and straddling channel boundaries)
        lengths = [max(1, M // 2) if M > 1 else 1, V, (F + 1) * V - 3]
        for L in lengths:
            for C, K in ((1, 1), (3, 5), (1, 64), (3, 64)):
                x, h = _rand(rng, (C, L)), _rand(rng, (K, M))
                got = bank.run(x, h, N, mode)
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
def test_filter_group_split_is_bit_exact(bank, N, M):
    """K = 200 on a signal of 20 workgroup tiles: the launch splits the filters into 100 groups of 2 (fir_filter_group_size); every
    row equals the K = 1 launch of its filter to the bit"""
    bank.check_group_split(N, M, 20 * (4096 // N) * (N - M + 1) - 7, tiles=20, plan=(2, 100))


@pytest.mark.parametrize("N", SIZES)
def test_prepared_spectra(bank, N):
    """smfft_fir_prepare = fft(pad(g)) / N within the per-FFT tolerances; a launch with NumPy-prepared spectra gives the library's result"""
    bank.check_prepared_spectra(N)


def test_caller_stream(bank):
    """prepare and launch on a stream from hipStreamCreate, then hipStreamSynchronize"""
    bank.check_caller_stream([(1024, 257)], C=2, K=9, L=50000)


def test_benchmark_form(bank):
    bank.check_benchmark_form(N=512, M=100, K=3, L=20000)


def test_output_offsets_beyond_two_to_the_31(bank):
    """C = 1, K = 64, L = 2^25 + 1000: 2.15e9 output elements (16 GiB); sampled windows of the last filter rows against np.convolve /
    np.correlate on the matching input slice"""
    N, M, K, L = 1024, 257, 64, (1 << 25) + 1000
    rng = np.random.default_rng(5)
    x = _rand(rng, (1, L))
    h = _rand(rng, (K, M))
    bank.check_output_offsets(x, h, N)


# ---- the grid-stride loop and the filter groups ------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_grid_stride_loop_with_wrapped_prefetch(bank, N, mode):
    """M = N - 1 (V = 2 outputs per segment), C = 3, K = 3: about 2.5 x 12288 tiles, so every workgroup runs two or three tiles and
    after its last filter prefetches the first filter's spectrum for its next tile.  S = 10240 F + 1 segments per channel (F = 4096 / N
    per tile): tiles straddle channel boundaries for N < 4096 and the last one is partial; L = 2 S - 1 leaves the last segment one
    output.  Every row against fp64."""
    bank.check_grid_stride_loop(N, mode)


@pytest.mark.parametrize("mode", MODES)
def test_grid_stride_loop_at_a_realistic_shape(sm, bank, mode):
    """N = 1024, M = 257, C = 3 channels of L = 16e6 samples, K = 2: 15,626 tiles, past the grid cap.  Sampled windows against
    np.convolve / np.correlate: the first and last of every (channel, filter) row (their segments' tiles straddle two channels), one in
    the middle, and the one where the grid-stride loop's second pass starts (tile 12288)."""
    N, M, C, K, L = 1024, 257, 3, 2, 16_000_000
    V, F = N - M + 1, 4096 // N
    S = -(-L // V)
    tiles = bank.tiles(L, C, N, M)
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
        bank.sampled_windows(dout, x, h, L, starts, mode, f"L=16e6 {mode}", W)
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
def test_uneven_filter_groups(bank, N, L, K, plan, mode):
    """M = N - 1 on 700 / 450 tiles: filter groups of the rule's size with a shorter last group, and a grid of fewer rows than the
    groups the rule asked for.  Every row equals the K = 1 launch of its filter (the same spectrum) to the bit and is within bounds
    against fp64."""
    bank.check_uneven_groups(N, L, K, plan, mode)

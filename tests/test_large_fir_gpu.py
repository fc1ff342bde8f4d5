"""The overlap-save FIR filter banks with N = 8192 / 16384 segments on an MI355X (smfft_large_fir_prepare / smfft_large_fir_launch,
smfft_amd.large_fir) against fp64 NumPy: the cases of tests/test_fir_gpu.py carried to these lengths -- both modes over a grid of taps,
channels, filters and signal lengths; K = 200 filters against 200 single-filter launches; the persistent loop several times round the
grid; the prepared spectra; a caller's stream; the benchmark form; 64-bit output offsets -- and the two neighbours still doing what
they did.

Tolerances per (channel, filter) row: those of tests/test_fir_gpu.py (relL2 <= 1e-6, max <= 5e-6, with its denominators)."""
import numpy as np
import pytest

from oracle.np_reference import MAX_ABS_TOL, REL_L2_TOL
from tests.fir_gpu_harness import GUARD, MODES, Bank, _check_rows, _rand, _reference

import large_fir_model as lfm  # noqa: E402  (tools/ is on the path once tests.fir_gpu_harness is imported)

pytestmark = pytest.mark.gpu

SIZES = [8192, 16384]


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    import smfft_amd.large  # noqa: F401  (sm.large: the persistent grid)
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def lf():
    from smfft_amd import large_fir
    large_fir.lib()
    return large_fir


@pytest.fixture(scope="module")
def bank(sm, lf):
    return Bank.large(sm, lf)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_filter_bank_matches_numpy(sm, lf, bank, N, mode):
    rng = np.random.default_rng(N + (mode == "correlate"))
    for M in (1, 17, N // 4 + 1, N - 1):
        V = N - M + 1
        # L < M; one segment; two segments per channel, the second three outputs short
        lengths = [max(1, M // 2) if M > 1 else 1, V, 2 * V - 3 if V > 2 else 1]
        for L in lengths:
            for C, K in ((1, 1), (3, 5), (1, 64), (3, 64)):
                x, h = _rand(rng, (C, L)), _rand(rng, (K, M))
                got = bank.run(x, h, N, mode)
                _check_rows(got, _reference(x, h, mode == "correlate"), f"N={N} {mode} M={M} L={L} C={C} K={K}", x, h)


def test_host_convenience(sm, lf):
    """fir(): 1-D and real inputs, the default transform length, the (C, K, L) result"""
    rng = np.random.default_rng(7)
    x = rng.standard_normal(50000).astype(np.float32)
    for M, N in ((65, 8192), (4097, 16384)):
        h = _rand(rng, (M,))
        assert lf.fir_fft_size(M) == N
        for mode in MODES:
            got = lf.fir(x, h, mode)
            assert got.shape == (1, 1, 50000) and got.dtype == np.complex64
            _check_rows(got, _reference(x[None].astype(np.complex64), h[None], mode == "correlate"), f"fir() {mode}", x[None], h[None])
    got = lf.fir(_rand(rng, (2, 30000)), _rand(rng, (3, 33)), fft_size=16384)
    assert got.shape == (2, 3, 30000)


@pytest.mark.parametrize("N,M", [(8192, 2049), (16384, 4097)])
def test_k_filters_equal_k_single_launches(bank, N, M):
    """K = 200 on a short signal (three segments): every row equals the K = 1 launch of its filter to the bit.  At 8192 the K = 200
    launch runs the held form -- on 256 CUs 67 filter groups of 3, the last of 2 (fir_filter_group_size(3, 200, CUs)) -- and the
    single-filter launches the recompute form."""
    bank.check_group_split(N, M, 3 * (N - M + 1) - 7)


@pytest.mark.parametrize("N", SIZES)
def test_prepared_spectra(bank, N):
    """smfft_large_fir_prepare = fft(pad(g)) / N within the per-FFT tolerances; a launch with NumPy-prepared spectra gives the library's
    result"""
    bank.check_prepared_spectra(N)


def test_prepare_more_filters_than_the_grid(sm, lf):
    """K = 700 filters at N = 8192: the prepare kernel's persistent loop wraps; sampled filters against fp64"""
    rng = np.random.default_rng(70)
    N, M, K = 8192, 33, 700
    assert K > sm.large.grid(N) > 0
    h = _rand(rng, (K, M))
    dh, dspec = sm.DeviceBuffer.from_host(h), sm.DeviceBuffer(K * N * 8)
    lf.prepare(dh.ptr, dspec.ptr, M, K, N, "correlate")
    assert sm.lib.smfft_synchronize() == 0
    got = dspec.to_host(np.complex64, (K, N))
    for k in (0, 1, 255, 256, 511, 512, 513, 699):
        want = lfm.spectra(h[k], N, True)[0]
        d = got[k] - want
        assert np.linalg.norm(d) / np.linalg.norm(want) <= REL_L2_TOL and np.max(np.abs(d)) / np.max(np.abs(want)) <= MAX_ABS_TOL, k
    dh.free()
    dspec.free()


def test_caller_stream(bank):
    """prepare and launch on a stream from hipStreamCreate, then hipStreamSynchronize"""
    bank.check_caller_stream([(8192, 2049), (16384, 4097)], C=2, K=9, L=100000)


@pytest.mark.parametrize("N", SIZES)
def test_benchmark_form(bank, N):
    bank.check_benchmark_form(N, M=1000, K=3, L=60000)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_persistent_loop_several_times_round_the_grid(sm, lf, bank, N, mode):
    """M = N - 1 (V = 2 outputs per segment), C = 3, K = 3, S = 301 segments per channel: 2709 units, more than five times the grid
    of 8192 and ten times that of 16384; L = 2 S - 1 leaves the last segment one output.  Every row against fp64."""
    M, C, K, S = N - 1, 3, 3, 301
    L = 2 * S - 1
    grid = sm.large.grid(N)
    assert 0 < 5 * grid <= C * S * K and lfm.Window(L, N, M, False).segments() == S
    rng = np.random.default_rng(12288 + N + (mode == "correlate"))
    x, h = _rand(rng, (C, L)), _rand(rng, (K, M))
    got = bank.run(x, h, N, mode)
    _check_rows(got, _reference(x, h, mode == "correlate"), f"persistent loop N={N} {mode}", x, h)


@pytest.mark.parametrize("N,M", [(8192, 2049), (16384, 4097)])
@pytest.mark.parametrize("mode", MODES)
def test_persistent_loop_at_a_realistic_shape(sm, lf, bank, N, M, mode):
    """C = 3 channels of L = 16e6 samples, K = 2: thousands of units on a grid of a few hundred.  Sampled windows against np.convolve /
    np.correlate: the first and last of every (channel, filter) row, one in the middle, and the one of the first unit of the grid's
    second round."""
    C, K, L = 3, 2, 16_000_000
    V = N - M + 1
    S = -(-L // V)
    grid = sm.large.grid(N)
    assert 0 < grid and C * S * K > 4 * grid
    rng = np.random.default_rng(16)
    x = rng.standard_normal((C, 2 * L), dtype=np.float32).view(np.complex64)
    h = _rand(rng, (K, M))
    W = 3000
    starts = [[0, L // 2 + 11, L - W] for _ in range(C)]
    c2, s2 = divmod(grid // K, S)                     # unit `grid` = (c2 S + s2) K + grid % K
    starts[c2].append(min(L - W, max(0, s2 * V - W // 2)))
    dx, dh = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer.from_host(h)
    dspec, dout = sm.DeviceBuffer(K * N * 8), sm.DeviceBuffer((C * K * L + GUARD) * 8)
    try:
        assert sm.lib.smfft_memset(dout.ptr, 0xFF, C * K * L * 8) == 0
        assert sm.lib.smfft_memset(dout.ptr + C * K * L * 8, 0x5A, GUARD * 8) == 0
        lf.prepare(dh.ptr, dspec.ptr, M, K, N, mode)
        lf.launch(dx.ptr, L, C, dspec.ptr, K, M, N, dout.ptr, mode)
        assert sm.lib.smfft_synchronize() == 0
        guard = np.empty(GUARD * 8, np.uint8)
        assert sm.lib.smfft_memcpy_d2h(guard.ctypes.data, dout.ptr + C * K * L * 8, GUARD * 8) == 0
        assert np.all(guard == 0x5A), "the kernel wrote past its output"
        bank.sampled_windows(dout, x, h, L, starts, mode, f"L=16e6 N={N} {mode}", W)
    finally:
        for b in (dx, dh, dspec, dout):
            b.free()


@pytest.mark.parametrize("N,M", [(8192, 2049), (16384, 4097)])
def test_output_offsets_beyond_two_to_the_31(bank, N, M):
    """C = 1, K = 64, L = 2^25 + 1000: 2.15e9 output elements (16 GiB); sampled windows of the last filter rows against np.convolve /
    np.correlate on the matching input slice"""
    K, L = 64, (1 << 25) + 1000
    rng = np.random.default_rng(5)
    x = rng.standard_normal((1, 2 * L), dtype=np.float32).view(np.complex64)
    h = _rand(rng, (K, M))
    bank.check_output_offsets(x, h, N)


def test_neighbours_keep_their_limits(sm, lf):
    """smfft_fir_launch still answers -1 above N = 4096 and serves 4096; smfft_large_launch still serves 8192 and rejects 4096"""
    for n in SIZES:
        assert sm.lib.smfft_fir_launch(None, 1000, 1, None, 1, 17, n, 0, None, None) == -1
        assert sm.lib.smfft_fir_prepare(None, 17, 1, n, 0, None, None) == -1
    rng = np.random.default_rng(1)
    x, h = _rand(rng, (1, 9000)), _rand(rng, (2, 1025))
    _check_rows(sm.fir(x, h, fft_size=4096), _reference(x, h, False), "smfft_fir at 4096", x, h)
    assert sm.large.lib().smfft_large_launch(None, None, 4096, 1, 0, None) == -1
    z = _rand(rng, (3, 8192))
    got = sm.large.c2c(z)
    want = np.fft.fft(z.astype(np.complex128), axis=1)
    assert np.linalg.norm(got - want) / np.linalg.norm(want) <= REL_L2_TOL

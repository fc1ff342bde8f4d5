"""The polyphase filter bank channelizer for N = 8192 / 16384 channels on an MI355X (smfft_large_pfb_*, smfft_amd.large_pfb) against the
fp64 model of tools/large_pfb_model.py: both modes at both lengths over a grid of taps per channel, prototypes, streams and frames;
several rounds of a small grid under both schedules; more pairs than the device's grid; a bare transform at the library's per-FFT
bounds; bit-identity across schedules, grids and stream splits; a caller's stream, the benchmark form, interior pointers, 64-bit
offsets; the host conveniences on two tones.

Every run goes through the guarded run of tests/pfb_gpu_harness.py: the output is prefilled with 0xFF (NaN) and followed by a guard of
0x5A that must stay untouched; the signal carries NaN before stream 0, after the last stream and in every stream's unread tail.  The
bounds are that module's row bounds (its docstring derives them): complex ||d||_2 / (sqrt(N) ||s||_2) <= 1e-6 and max <= 5e-6, power
L1 <= 2e-6 and max <= 1e-5.  An fp32 emulation on the CPU (sequential fp32 weighted sum, complex64 FFT; N in {8192, 16384}, P in
{1, 8, 32}, Gaussian and all-ones taps) stays at <= 3.7e-8, 9.1e-8, 1.2e-7 and 1.8e-7 of the four."""
import numpy as np
import pytest

from tests import pfb_gpu_checks as checks
from tests import pfb_gpu_harness as gh

pytestmark = pytest.mark.gpu

SIZES = [8192, 16384]
TAPS = gh.TAPS
STRIDE, BLOCKED = 1, 2


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def lp():
    bank = gh.Bank("large_pfb")
    bank.lib
    yield bank
    print(bank.worst.rows_line())


def _tuned(lp, schedule, max_workgroups):
    """a launcher for the bank's run: smfft_large_pfb_launch_tuned with this schedule and grid"""
    lib = lp.lib
    return lambda *a: lib.launch_tuned(*a[:-1], schedule=schedule, max_workgroups=max_workgroups, power=a[-1])


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("P", TAPS)
def test_filter_bank_matches_the_model(sm, lp, P):
    """both lengths x every prototype x (C, F) in {(1, 1), (1, 3), (3, 5)} (one pair; one stream; pairs of three streams on one grid),
    ragged tails, both modes, Gaussian signals"""
    for N in SIZES:
        checks.check_filter_bank_matches_the_model(sm, lp, N, P, ((1, 1, 0), (1, 3, N - 1), (3, 5, N // 2 + 3)))


def test_multi_round_through_launch_tuned(sm, lp):
    """74 pairs of two streams on a grid of 16: four rounds and a ragged one of ten, at both lengths under either schedule"""
    P, C, F = 4, 2, 37
    for N in SIZES:
        rng = np.random.default_rng([N, 3])
        x, h = lp.rand(rng, (C, lp.length(N, P, F, 100))), lp.taps(rng, N, P)
        for schedule in (STRIDE, BLOCKED):
            lp.check_both_modes(sm, x, h, N, f"N={N} schedule={schedule} grid 16, 74 pairs", launcher=_tuned(lp, schedule, 16))


def test_full_grid(sm, lp):
    """one default launch per length with more pairs than the device's grid: a full round and a ragged one of half the grid and one"""
    from smfft_amd import large
    for N in SIZES:
        grid = large.grid(N)
        rng = np.random.default_rng([N, 5])
        P, F = 4, grid + grid // 2 + 1
        x, h = lp.rand(rng, (1, lp.length(N, P, F, 9))), lp.lib.prototype(N, P)
        lp.check_rows(lp.run(sm, x, h, N, False), x, h, N, False, f"N={N} full grid {grid}, {F} pairs")


def test_one_tap_of_ones_is_a_bare_transform(sm, lp):
    """P = 1, h = 1: the library's per-FFT bounds (oracle/np_reference.py)"""
    for N in SIZES:
        checks.check_one_tap_of_ones_is_a_bare_transform(sm, lp, N, 5, 5)


# ------------------------------------------------------------------------------------------------ bit identity
def test_every_schedule_and_grid_gives_the_same_bits(sm, lp):
    """74 pairs: one workgroup; grids of 8, 16 and 24 (multiples of 8); 20 (rounded down to 16 by the blocked schedule); the device's"""
    for N, P, power in ((8192, 8, False), (16384, 4, True)):
        rng = np.random.default_rng(N + P)
        C, F = 2, 37
        x, h = lp.rand(rng, (C, lp.length(N, P, F, 9))), lp.lib.prototype(N, P)
        base = lp.run(sm, x, h, N, power)
        for schedule in (STRIDE, BLOCKED):
            for max_workgroups in (1, 8, 16, 20, 24, 0):
                got = lp.run(sm, x, h, N, power, launcher=_tuned(lp, schedule, max_workgroups))
                assert np.array_equal(gh.bits(got), gh.bits(base)), f"N={N} P={P} schedule={schedule} max_workgroups={max_workgroups}"
        lp.check_rows(base, x, h, N, power, f"schedules N={N}")


def test_three_streams_equal_three_launches(sm, lp):
    for N, P in ((8192, 4), (16384, 2)):
        checks.check_three_streams_equal_three_launches(sm, lp, N, P, 5, 5)


# ------------------------------------------------------------------------------------------------ the ABI's corners
def test_caller_stream(sm, lp):
    checks.check_caller_stream(sm, lp, 8192, 8, 2, 7, " power")


def test_benchmark_adds_to_its_total(sm, lp):
    checks.check_benchmark_adds_to_its_total(sm, lp, 16384, 4, 1, 40, 1)


def test_interior_pointers(sm, lp):
    """signal, taps and output at odd element offsets inside their buffers (8-byte aligned, 4 for taps and the power output)"""
    checks.check_interior_pointers(sm, lp, ((8192, 4, 3), (16384, 2, 3)), 3, (3, 1, 5), (1, 3, 1))


def test_offsets_beyond_two_to_the_31(sm, lp):
    """N = 16384, P = 4, C = 3, F = 43691: 2^31 + 163855 input elements and 2^31 + 16384 output elements in one launch (17 GiB in, 17 GiB
    out, as in tests/test_pfb_gpu.py's test of this name: the same output size, and 141317 input elements -- 1.1 MB -- more, because a frame
    here is 16384 elements), complex mode, on the periodic device signal of tests/pfb_gpu_harness.py (PeriodicLaunch).  Sampled
    pairs -- the first, the last, the two either side of output element 2^31 and the two either side of each stream boundary --
    against the model on the input slice copied back."""
    N, P, C = 16384, 4, 3
    F = 43691
    split = (1 << 31) // N                                   # the pair that holds output element 2^31: the last one
    assert C * F * N == (1 << 31) + N and split == C * F - 1 and 2 * F < split - 1
    checks.check_offsets_beyond_two_to_the_31(sm, lp, N, P, C, F, [0, split - 1, split, F - 1, F, 2 * F - 1, 2 * F])


# ------------------------------------------------------------------------------------------------ the host conveniences
def test_channelize_and_prototype_on_two_tones(sm, lp):
    """a unit tone at channel 100.37 plus one of a tenth of its amplitude at channel N/2 + 7.5, through prototype() and channelize(): parity
    with the model in both modes (the tones' power bounds of tests/pfb_gpu_harness.py), and the leakage of the strong tone alone, from the
    device's power output, against the model's figure for P (tests/pfb_gpu_harness.py, LEAKAGE).  With E = 2e-6 ||y||_2 sqrt(N) ||s||_2
    the bound on the L1 error of a power row, p the reference power in channel 100 and S the row's total, leakage = (S - p) / p moves
    by at most E / p + S E / p^2 <= 2 E / p (1 + leakage), which is the tolerance; the reference is the model on the same float32
    inputs, itself within 1 % of the figure."""
    lpm, LEAKAGE = lp.model, gh.LEAKAGE
    frames = 6
    for N, P in ((N, P) for N in SIZES for P in (2, 8, 32)):
        t = np.arange((frames + P - 1) * N + 13)
        strong = np.exp(2j * np.pi * 100.37 * t / N)
        both = (strong + 0.1 * np.exp(2j * np.pi * (N / 2 + 7.5) * t / N)).astype(np.complex64)
        h = checks.check_two_tones_parity(sm, lp, N, P, both, frames)
        # the strong tone alone
        strong32 = strong.astype(np.complex64)
        refs = lpm.pfb(strong32, h, N)
        refsp = refs.real ** 2 + refs.imag ** 2
        leak_ref = lpm.leakage_of(refsp, 100)
        assert np.all(np.abs(leak_ref - LEAKAGE[P]) <= 0.01 * LEAKAGE[P]), (N, P, leak_ref, LEAKAGE[P])
        leak = lpm.leakage_of(lp.lib.channelize(strong32, h, N, power=True), 100)
        E = gh.POWER_L1 * np.linalg.norm(refs, axis=-1) * np.sqrt(N) * np.linalg.norm(lpm.scale(strong32, h, N), axis=-1)
        tol = 2 * E / refsp[..., 100] * (1 + leak_ref)
        print(f"tones N={N} P={P}: leakage {leak.max():.3g}, model {leak_ref.max():.3g}, figure {LEAKAGE[P]:.3g}, tolerance {tol.max():.3g}")
        assert np.all(np.abs(leak - leak_ref) <= tol), (N, P, leak, leak_ref, tol)

"""The polyphase filter bank channelizer on an MI355X (smfft_pfb_*, smfft_amd.pfb) against the fp64 model of tools/pfb_model.py: both
modes at every length over a grid of taps per channel, prototypes, streams and frames; a bare transform at the library's per-FFT
bounds; bit-identity across schedules and across stream splits; a caller's stream, the benchmark form, interior pointers, 64-bit
offsets; the host conveniences on two tones.

Every run goes through the guarded run of tests/pfb_gpu_harness.py (a NaN-fenced signal into a 0xFF-prefilled output between guards of
0x5A); that module's docstring derives the row bounds: complex ||got - ref||_2 / (sqrt(N) ||s||_2) <= 1e-6 and max <= 5e-6, power
L1 <= 2e-6 and max <= 1e-5, and the tones' power bounds of test_channelize_and_prototype_on_two_tones.  The tests' bodies are shared with
the real bank: tests/pfb_gpu_checks.py."""
import numpy as np
import pytest

from tests import pfb_gpu_checks as checks
from tests import pfb_gpu_harness as gh

pytestmark = pytest.mark.gpu

SIZES, TAPS = gh.SIZES, gh.TAPS


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def pfb():
    bank = gh.Bank("pfb")
    bank.lib
    yield bank
    print(bank.worst.rows_line())


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("P", TAPS)
def test_filter_bank_matches_the_model(sm, pfb, N, P):
    """every prototype x (C, F) in {(1, 1), (1, 4096/N + 1), (3, 2 4096/N + 1), (2, 1000)} (one frame; a partial second tile; tiles
    straddling streams; many tiles), ragged tails, both modes, Gaussian signals"""
    per = 4096 // N
    checks.check_filter_bank_matches_the_model(sm, pfb, N, P, ((1, 1, 0), (1, per + 1, N - 1), (3, 2 * per + 1, N // 2 + 3), (2, 1000, 17)))


@pytest.mark.parametrize("N", SIZES)
def test_one_tap_of_ones_is_a_bare_transform(sm, pfb, N):
    """P = 1, h = 1: the library's per-FFT bounds (oracle/np_reference.py)"""
    checks.check_one_tap_of_ones_is_a_bare_transform(sm, pfb, N, 3 * (4096 // N) + 1, 5)


# ------------------------------------------------------------------------------------------------ bit identity
@pytest.mark.parametrize("N,P,power", [(1024, 8, False), (4096, 4, True), (256, 16, False)])
def test_every_schedule_gives_the_same_bits(sm, pfb, N, P, power):
    """15000 tiles: more runs than any grid for R = 1, 3 and 16 (the outer stride runs), one run for R above the tile count"""
    checks.check_every_schedule_gives_the_same_bits(sm, pfb, N, P, power, tiles=15000, tail=9)


@pytest.mark.parametrize("N,P", [(512, 4), (2048, 2)])
def test_three_streams_equal_three_launches(sm, pfb, N, P):
    checks.check_three_streams_equal_three_launches(sm, pfb, N, P, 2 * (4096 // N) + 1, 5)       # tiles straddle the streams


# ------------------------------------------------------------------------------------------------ the ABI's corners
def test_caller_stream(sm, pfb):
    checks.check_caller_stream(sm, pfb, 1024, 8, 2, 37, ", power")


def test_benchmark_adds_to_its_total(sm, pfb):
    checks.check_benchmark_adds_to_its_total(sm, pfb, 2048, 4, 1, 300, 1)


def test_interior_pointers(sm, pfb):
    """signal, taps and output at odd element offsets inside their buffers (8-byte aligned, 4 for taps and the power output)"""
    checks.check_interior_pointers(sm, pfb, [(N, P, 4096 // N + 2) for N, P in ((256, 4), (4096, 2))], 3, (3, 1, 5), (1, 3, 1))


def test_offsets_beyond_two_to_the_31(sm, pfb):
    """N = 1024, P = 4, C = 2, F = 2^20 + 8: 2^31 + 22538 input elements and 2^31 + 16384 output elements in one launch (17 GiB in, 17 GiB
    out), complex mode, on the periodic device signal of tests/pfb_gpu_harness.py (PeriodicLaunch).  Sampled frames -- the first, the
    last, the two either side of output element 2^31 and the two either side of the stream boundary -- against the model on the input
    slice copied back."""
    N, P, C = 1024, 4, 2
    F = (1 << 20) + 8
    split = (1 << 31) // N                                   # the pair that holds output element 2^31
    assert F < split - 1 and split < C * F - 1
    checks.check_offsets_beyond_two_to_the_31(sm, pfb, N, P, C, F, [0, C * F - 1, split - 1, split, F - 1, F])


# ------------------------------------------------------------------------------------------------ the host conveniences
@pytest.mark.parametrize("N", [256, 1024, 4096])
def test_channelize_and_prototype_on_two_tones(sm, pfb, N):
    """a unit tone at channel 100.37 plus one of a tenth of its amplitude at channel N/2 + 7.5, through prototype() and channelize(): parity
    with the model in both modes, and the strong tone alone leaks less from the device's power output than from the rectangular
    window of a plain transform of one frame (smfft_amd.c2c)"""
    t = np.arange(40 * N + 13)
    strong = np.exp(2j * np.pi * 100.37 * t / N)
    both = (strong + 0.1 * np.exp(2j * np.pi * (N / 2 + 7.5) * t / N)).astype(np.complex64)
    rect = np.abs(sm.c2c(strong[:N].astype(np.complex64)[None, :])[0].astype(np.complex128)) ** 2
    rect = gh.leakage(rect, 100)
    for P in (2, 4, 8, 16, 32):
        h = checks.check_two_tones_parity(sm, pfb, N, P, both, 41 - P)
        leak = gh.leakage(pfb.lib.channelize(strong.astype(np.complex64), h, N, power=True), 100)
        print(f"tones N={N} P={P}: leakage {leak.max():.3g} against {rect:.3g} of the plain transform")
        assert leak.max() < rect, (N, P, leak.max(), rect)

"""The polyphase filter bank channelizer for real streams on an MI355X (smfft_pfb_real_*, smfft_amd.pfb_real) against the fp64 model of
tools/pfb_real_model.py: both modes at every length over a grid of taps per channel, prototypes, streams and frames; a bare R2C at the
library's per-FFT bounds; agreement with the shipped complex bank at 2N channels; bit-identity across schedules and across stream
splits; a caller's stream, the benchmark form, interior pointers; the host conveniences on two tones.

Every run goes through the guarded run of tests/pfb_gpu_harness.py on float signals: the output is prefilled with 0xFF (NaN) and followed
by a 4096-element guard of 0x5A that must stay untouched; the signal buffer carries NaN in 4096 floats before stream 0, after stream
C - 1, and in every stream's unread tail [(F + P - 1) 2N, L), so that a read outside the contract shows up as a non-finite output.

Tolerances, per output spectrum (one (c, f) row): the complex bank's metrics and bounds (tests/pfb_gpu_harness.py) with the frame's 2N real
samples in the place of its N complex ones.  With s[n] = sum_p |h[2 p N + n]| |x[(f + p) 2N + n]|, n < 2N, the scale the fp32
accumulation rounds at (by Parseval the whole 2N-point spectrum has norm <= sqrt(2N) ||s||, and its N + 1 output values no more):
  complex mode, on the N + 1 values X[0 ... N]: ||got - ref||_2 / (sqrt(2N) ||s||_2) <= 1e-6  and
                max|got - ref| / max(max|ref|, ||s||_2) <= 5e-6;
  power mode, Gaussian signals, on the N values: ||got - ref||_1 / ||ref||_1 <= 2e-6 and max|got - ref| / max(ref) <= 1e-5;
  power mode, tones (the branches of an off-centre tone cancel): the same derivation before its last step, as in tests/pfb_gpu_harness.py.
Element 0 of every row is checked on its own as well: both of its components against (X[0], X[N]) within the row's max bound, and the
DC power against X[0]^2 within the row's power max bound.
A sequential fp32 emulation (weighted sum, complex64 FFT of the packed sequence, split in complex64; 2N in {512, 2048, 8192}, P in
{1, 4, 32}, Gaussian signal, Hamming-sinc prototype) stays at 9.6e-8, 2.1e-7, 1.9e-7 and 3.5e-7 of these four.
The tests' bodies are shared with the complex bank: tests/pfb_gpu_checks.py."""
import numpy as np
import pytest

from tests import pfb_gpu_checks as checks
from tests import pfb_gpu_harness as gh

pytestmark = pytest.mark.gpu

SIZES, TAPS = gh.SIZES, gh.TAPS
ROW_REL_L2, ROW_MAX = gh.ROW_REL_L2, gh.ROW_MAX


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def pr():
    bank = gh.Bank("pfb_real")
    bank.lib
    yield bank
    print(bank.worst.rows_line())


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("P", TAPS)
def test_filter_bank_matches_the_model(sm, pr, N, P):
    """every prototype x (C, F) in {(1, 1), (1, 4096/N + 1), (3, 2 4096/N + 1), (2, 300)} (one frame; a partial second tile; tiles
    straddling streams; many tiles), ragged even tails, both modes, Gaussian signals"""
    per = 4096 // N
    checks.check_filter_bank_matches_the_model(sm, pr, N, P, ((1, 1, 0), (1, per + 1, 2 * N - 2), (3, 2 * per + 1, N + 6), (2, 300, 18)))


@pytest.mark.parametrize("N", SIZES)
def test_one_tap_of_ones_is_a_bare_r2c(sm, pr, N):
    """P = 1, h = 1: np.fft.rfft of every frame at the library's per-FFT bounds (oracle/np_reference.py)"""
    checks.check_one_tap_of_ones_is_a_bare_transform(sm, pr, N, 3 * (4096 // N) + 1, 6)


@pytest.mark.parametrize("N", [256, 512, 1024, 2048])
def test_agrees_with_the_complex_bank_of_2n_channels(sm, pr, N):
    """channels 1 ... N - 1 against smfft_pfb_launch with 2N channels on x + 0j, within the sum of both kernels' bounds (each is within
    its own of the fp64 model, and the two models are the same numbers: tests/test_pfb_real_cpu.py)"""
    from smfft_amd import pfb
    rng = np.random.default_rng(3 * N)
    P, C, F = 4, 2, 4096 // N + 3
    x, h = pr.rand(rng, (C, pr.length(N, P, F, 10))), pr.lib.prototype(N, P)
    got = pr.run(sm, x, h, N, False)
    other = pfb.channelize(x.astype(np.complex64), h, 2 * N)
    assert other.shape == (C, F, 2 * N)
    d = got[..., 1:].astype(np.complex128) - other[..., 1:N]
    ref, s = pr.reference(x, h, N)
    sn = np.linalg.norm(s, axis=-1)
    l2 = np.linalg.norm(d, axis=-1) / (np.sqrt(2 * N) * sn)
    mx = np.abs(d).max(axis=-1) / np.maximum(np.abs(ref).max(axis=-1), sn)
    print(f"N={N}: against the complex bank relL2 {l2.max():.3e} (bound {2 * ROW_REL_L2}) max {mx.max():.3e} (bound {2 * ROW_MAX})")
    assert l2.max() <= 2 * ROW_REL_L2 and mx.max() <= 2 * ROW_MAX


# ------------------------------------------------------------------------------------------------ bit identity
@pytest.mark.parametrize("N,P,power", [(1024, 8, False), (4096, 4, True), (256, 16, False)])
def test_every_schedule_gives_the_same_bits(sm, pr, N, P, power):
    """3000 tiles: more runs than any grid for R = 1 and 3 (the outer stride runs), fewer for 16, one run for R above the tile count"""
    checks.check_every_schedule_gives_the_same_bits(sm, pr, N, P, power, tiles=3000, tail=10)


@pytest.mark.parametrize("N,P", [(512, 4), (2048, 2)])
def test_three_streams_equal_three_launches(sm, pr, N, P):
    checks.check_three_streams_equal_three_launches(sm, pr, N, P, 2 * (4096 // N) + 1, 6)       # tiles straddle the streams


# ------------------------------------------------------------------------------------------------ the ABI's corners
def test_caller_stream(sm, pr):
    checks.check_caller_stream(sm, pr, 1024, 8, 2, 37, ", power")


def test_benchmark_adds_to_its_total(sm, pr):
    checks.check_benchmark_adds_to_its_total(sm, pr, 2048, 4, 1, 300, 2)


def test_interior_pointers(sm, pr):
    """signal and taps an even number of floats inside their buffers (8-byte aligned), the output at odd element offsets (8-byte
    aligned in complex mode, 4 in power mode)"""
    checks.check_interior_pointers(sm, pr, [(N, P, 4096 // N + 2) for N, P in ((256, 4), (4096, 2))], 6, (6, 2, 5), (2, 10, 1))


# ------------------------------------------------------------------------------------------------ the host conveniences
@pytest.mark.parametrize("N", [256, 1024, 4096])
def test_channelize_and_prototype_on_two_tones(sm, pr, N):
    """a unit cosine at channel 100.37 plus one of a tenth of its amplitude at channel N/2 + 7.5 (channel k = k cycles per 2N samples),
    through prototype() and channelize(): parity with the model in all three output forms, and the strong tone alone leaks less from
    the device's power output than from the rectangular window of a plain rfft of one frame, the less the longer the prototype"""
    t = np.arange(40 * 2 * N + 26)
    strong = np.cos(2 * np.pi * 100.37 * t / (2 * N))
    both = (strong + 0.1 * np.cos(2 * np.pi * (N / 2 + 7.5) * t / (2 * N))).astype(np.float32)
    rect = gh.leakage(np.abs(np.fft.rfft(strong[:2 * N].astype(np.float32).astype(np.float64))[:N]) ** 2, 100)
    leaks = []
    for P in (2, 4, 8, 16, 32):
        h = checks.check_two_tones_parity(sm, pr, N, P, both, 41 - P)
        leak = gh.leakage(pr.lib.channelize(strong.astype(np.float32), h, N, power=True), 100)
        print(f"tones N={N} P={P}: leakage {leak.max():.3g} against {rect:.3g} of the plain transform")
        assert leak.max() < rect, (N, P, leak.max(), rect)
        leaks.append(leak.max())
    assert all(b < a for a, b in zip(leaks, leaks[1:])), leaks

"""tests/pfb_gpu_harness.py without a device: the guarded run and the row checks that hold the filter bank kernels to their buffer contract
and their bounds are held to what they claim.  smfft_amd is stood in for by numpy memory (tests/host_device.py: DeviceBuffer, smfft_memset,
smfft_synchronize), a launch by a Python function that reads and writes through the pointers it is given.

The guarded run, in the complex, the real and the integrated-spectra (T = 2) layout at N = 256, P = 2, C = 2, F = 3 with a ragged tail:
an honest launcher that writes the fp64 model's rows passes; one element written past the output, one before an offset output, a last
row left unwritten, the first sample of a stream's unread tail or the first sample after the last stream added into a last frame
each fail, with the message that names the fault.
The row checks, at (N, P) = (256, 4): the model's rows plus a perturbation of a quarter of the bound, rounded to fp32, pass; the same at
twice the bound fails (rounding the reference to fp32 costs at most 6e-8 of these scales).  The real bank's Nyquist component alone,
moved by twice the row's max bound, fails, and the message carries the element-0 figure."""
import re

import numpy as np
import pytest

from tests import pfb_gpu_harness as gh
from tests.host_device import HOST
from tests.host_device import at as _at

N, P, C, F, T = 256, 2, 2, 3, 2


# ---- the three layouts ------------------------------------------------------------------------------------------------------------------
class Layout:
    """one of the three output layouts: its signal, its guarded run, and a launcher that writes the model's rows after `spoil` has had
    the rows and the launch's view of the signal"""

    def __init__(self, name):
        self.name, self.real, self.spec = name, "real" in name, "spec" in name
        self.bank = None if self.spec else gh.Bank("pfb_real" if self.real else "pfb")
        self.spectra = gh.Spectra(None) if self.spec else None
        rng = np.random.default_rng(7)
        self.x = gh.rand(rng, (C, gh.length(N, P, F, 6, self.real)), self.real)
        self.h = rng.standard_normal(P * gh.chunk(N, self.real)).astype(np.float32)
        self.rows = F // T if self.spec else F
        self.used = (self.rows * (T if self.spec else 1) + P - 1) * gh.chunk(N, self.real)

    def model_rows(self, x, power):
        if self.spec:
            return self.spectra.model.integrate(x, self.h, N, T, self.real)[0].astype(np.float32)
        ref = self.bank.transform(x, self.h, N)
        if power:
            return (gh.prm.power(ref) if self.real else ref.real ** 2 + ref.imag ** 2).astype(np.float32)
        return (gh.prm.pack(ref) if self.real else ref).astype(np.complex64)

    def run(self, power=False, spoil=None, **kw):
        """the guarded run of this layout with a launcher that computes the model's rows from the memory it is pointed at, lets
        spoil(rows, d_output, signal) change them or write elsewhere, and stores what is left (NaN rows are not stored)"""
        def launcher(d_signal, L, C_, d_taps, N_, P_, *rest):
            d_output = rest[-2] if not self.spec else rest[-1]
            signal = _at(d_signal, self.x.dtype, C_ * L + 1)              # + 1: the first sample after the last stream
            taps = _at(d_taps, np.float32, self.h.size)
            assert np.array_equal(taps, self.h)
            rows = self.model_rows(signal[:C_ * L].reshape(C_, L), power)
            keep = np.ones(rows.shape[:2], bool)
            if spoil is not None:
                spoil(rows, keep, d_output, signal)
            out = _at(d_output, rows.dtype, rows.size).reshape(rows.shape)
            out[keep] = rows[keep]
        if self.spec:
            return self.spectra.run(HOST, self.x, self.h, N, T, self.real, launcher=launcher, **kw)
        return self.bank.run(HOST, self.x, self.h, N, power, launcher=launcher, **kw)


LAYOUTS = ("complex", "real", "complex spec", "real spec")


@pytest.fixture(scope="module", params=LAYOUTS)
def layout(request):
    return Layout(request.param)


def test_an_honest_launcher_passes(layout):
    for power in ((False,) if layout.spec else (False, True)):
        for offsets in ({}, {"in_off": 2, "tap_off": 2, "out_off": 3}):
            got = layout.run(power, **offsets)
            assert got.shape == (C, layout.rows, N) and np.array_equal(gh.bits(got), gh.bits(layout.model_rows(layout.x, power)))


def test_a_write_past_the_output_fails(layout):
    def past(rows, keep, d_output, signal):
        _at(d_output, rows.dtype, rows.size + 1)[-1] = 0
    with pytest.raises(AssertionError, match="wrote past its output"):
        layout.run(spoil=past)


def test_a_write_before_an_offset_output_fails(layout):
    def before(rows, keep, d_output, signal):
        _at(d_output - rows.itemsize, rows.dtype, 1)[0] = 0
    with pytest.raises(AssertionError, match="wrote before its output"):
        layout.run(spoil=before, out_off=3)


def test_an_unwritten_last_row_fails(layout):
    def lazy(rows, keep, d_output, signal):
        keep[-1, -1] = False
    with pytest.raises(AssertionError, match="outputs left unwritten, or a sample read outside the contract"):
        layout.run(spoil=lazy)


@pytest.mark.parametrize("stream", (0, C - 1))
def test_a_read_of_a_streams_unread_tail_fails(layout, stream):
    """the first sample a stream's launch may not read, added into that stream's last frame"""
    L = layout.x.shape[1]
    assert layout.used < L

    def greedy(rows, keep, d_output, signal):
        rows[stream, -1, 0] += signal[stream * L + layout.used].real
    with pytest.raises(AssertionError, match="outputs left unwritten, or a sample read outside the contract"):
        layout.run(spoil=greedy)


def test_a_read_after_the_last_stream_fails(layout):
    L = layout.x.shape[1]

    def greedy(rows, keep, d_output, signal):
        rows[-1, -1, 0] += signal[C * L].real
    with pytest.raises(AssertionError, match="outputs left unwritten, or a sample read outside the contract"):
        layout.run(spoil=greedy)


def test_a_read_before_the_first_stream_fails(layout):
    def greedy(rows, keep, d_output, signal):
        rows[0, 0, 0] += _at(signal.ctypes.data - signal.itemsize, signal.dtype, 1)[0].real
    with pytest.raises(AssertionError, match="outputs left unwritten, or a sample read outside the contract"):
        layout.run(spoil=greedy)


def test_non_finite_outputs_pass_only_where_the_caller_says_so(layout):
    def lazy(rows, keep, d_output, signal):
        keep[0, 0] = False
    got = layout.run(spoil=lazy, finite=False)
    assert np.all(np.isnan(got[0, 0].view(np.float32))) and np.all(np.isfinite(got[1:].view(np.float32)))


# ---- the row checks ---------------------------------------------------------------------------------------------------------------------
ROWS_P = 4


def _case(real):
    rng = np.random.default_rng(11 + real)
    bank = gh.Bank("pfb_real" if real else "pfb")
    x = bank.rand(rng, (2, bank.length(N, ROWS_P, 5, 0)))
    h = bank.taps(rng, N, ROWS_P)
    return rng, bank, x, h, bank.reference(x, h, N)


def _unit_rows(rng, shape, real_ends):
    """rows of unit norm whose elements all have the same magnitude and a random phase (a random sign at both ends with real_ends)"""
    d = np.exp(2j * np.pi * rng.random(shape))
    if real_ends:
        d[..., 0], d[..., -1] = np.sign(d[..., 0].real), np.sign(d[..., -1].real)
    return d / np.sqrt(shape[-1])


def _signs(rng, shape):
    return rng.integers(0, 2, shape) * 2.0 - 1.0


@pytest.mark.parametrize("real", (False, True))
def test_complex_rows_pass_within_the_bound_and_fail_beyond_it(real, capsys):
    rng, bank, x, h, (ref, s) = _case(real)
    d = _unit_rows(rng, ref.shape, real) * (gh.ROW_REL_L2 * np.sqrt(bank.chunk(N)) * np.linalg.norm(s, axis=-1))[..., None]
    rows = gh.prm.pack if real else (lambda y: y)
    bank.check(rows(ref + 0.25 * d).astype(np.complex64), ref, s, False, "a quarter")
    assert 0.24 * gh.ROW_REL_L2 < bank.worst["l2"] < 0.26 * gh.ROW_REL_L2
    with pytest.raises(AssertionError, match="twice: relL2=2.0"):
        bank.check(rows(ref + 2 * d).astype(np.complex64), ref, s, False, "twice")
    assert "a quarter: relL2 2.5" in capsys.readouterr().out


@pytest.mark.parametrize("real", (False, True))
def test_power_rows_pass_within_the_bound_and_fail_beyond_it(real):
    rng, bank, x, h, (ref, s) = _case(real)
    refp = gh.prm.power(ref) if real else ref.real ** 2 + ref.imag ** 2
    d = _signs(rng, refp.shape) * gh.POWER_L1 * refp
    bank.check((refp + 0.25 * d).astype(np.float32), ref, s, True, "a quarter")
    assert 0.24 * gh.POWER_L1 < bank.worst["pl1"] < 0.26 * gh.POWER_L1
    with pytest.raises(AssertionError, match="twice: L1=4.0"):
        bank.check((refp + 2 * d).astype(np.float32), ref, s, True, "twice")


@pytest.mark.parametrize("real", (False, True))
def test_integrated_spectra_pass_within_the_bound_and_fail_beyond_it(real):
    rng, bank, x, h, _ = _case(real)
    spectra = gh.Spectra(None)
    ref, m = spectra.model.integrate(x, h, N, T, real)
    d = _signs(rng, ref.shape) * (gh.POWER_L1 + gh.gamma(T)) * ref
    spectra.check((ref + 0.25 * d).astype(np.float32), x, h, N, T, real, "a quarter")
    assert 0.24 < spectra.worst["l1"] < 0.26
    with pytest.raises(AssertionError, match="twice: L1 2.0"):
        spectra.check((ref + 2 * d).astype(np.float32), x, h, N, T, real, "twice")


def test_the_real_banks_nyquist_component_is_held_on_its_own():
    """only Im of element 0 -- X[N] -- moves, by twice the row's max bound: the element-0 figure of the message shows it"""
    rng, bank, x, h, (ref, s) = _case(True)
    denom = np.maximum(np.abs(ref).max(axis=-1), np.linalg.norm(s, axis=-1))
    got = gh.prm.pack(ref)
    got[..., 0] += 1j * 2 * gh.ROW_MAX * denom
    with pytest.raises(AssertionError) as failure:
        bank.check(got.astype(np.complex64), ref, s, False, "nyquist")
    assert float(re.search(r"element 0=(\S+)", str(failure.value)).group(1)) > 1.9 * gh.ROW_MAX
    # and the DC power alone: the power of X[0], no Nyquist in it
    gotp = gh.prm.power(ref)
    gotp[..., 0] += 2 * gh.POWER_MAX * gotp.max(axis=-1)
    with pytest.raises(AssertionError) as failure:
        bank.check(gotp.astype(np.float32), ref, s, True, "dc")
    assert float(re.search(r"element 0=(\S+)", str(failure.value)).group(1)) > 1.9 * gh.POWER_MAX


def test_each_owner_has_its_own_worst_figures():
    a, b = gh.Bank("pfb"), gh.Bank("large_pfb")
    rng, bank, x, h, (ref, s) = _case(False)
    a.check(ref.astype(np.complex64), ref, s, False, "fp32 rounding")
    assert 0 < a.worst["l2"] < 1e-7 and not b.worst and "worst seen: complex relL2 0.000e+00" in b.worst.rows_line()

"""tests/fir_gpu_harness.py without a device: the guarded run and the row check that hold the FIR kernels to their buffer contract and
their bounds are held to what they claim.  smfft_amd is stood in for by numpy memory (tests/host_device.py), a bank by a prepare that
writes the fp64 model's spectra and a launch that writes the fp64 model's rows (tools/fir_plan_model.overlap_save for the complex layout,
tools/fir_real_model.overlap_save_pairs for the real one) through the pointers they are given.

At N = 256, M = 65, C = 2, K = 3, L = 2 V + 1 (three segments, the last of one output; in the real layout a pair and a lone segment),
both modes: the honest bank passes the guarded run and the row check; one element written past the output or a last output left
unwritten fail the run, and a row moved by twice the relL2 bound or one output moved by twice the max bound fails the check, each with
the message that names the fault; a quarter of either bound, rounded to fp32, passes (the rounding costs at most 6e-8 of these scales)."""
import re

import numpy as np
import pytest

from tests import fir_gpu_harness as gh
from tests.host_device import HOST
from tests.host_device import at as _at

import fir_plan_model as fm  # noqa: E402  (tools/ is on the path once tests.fir_gpu_harness is imported)
import fir_real_model as frm  # noqa: E402

N, M, C, K = 256, 65, 2, 3
L = 2 * (N - M + 1) + 1


class Layout:
    """the complex or the real layout: its signal and taps, and a bank whose launch writes the model's rows after `spoil` has had them"""

    def __init__(self, real):
        self.real = real
        rng = np.random.default_rng(7 + real)
        self.bank = gh.Bank(HOST, real, self.prepare, self.launch)
        self.x, self.h = self.bank.rand(rng, (C, L)), self.bank.rand(rng, (K, M))
        self.spoil = None

    def model_rows(self, x, correlate):
        return (frm.overlap_save_pairs if self.real else fm.overlap_save)(x, self.h, N, correlate)

    def prepare(self, d_taps, d_spectra, n_taps, n_filters, n, mode, stream=0):
        taps = _at(d_taps, self.bank.dtype, n_filters * n_taps).reshape(n_filters, n_taps)
        _at(d_spectra, np.complex64, n_filters * n)[:] = fm.spectra(taps, n, mode == "correlate").astype(np.complex64).reshape(-1)

    def launch(self, d_signal, length, n_channels, d_spectra, n_filters, n_taps, n, d_output, mode, stream=0):
        assert (n_channels, n_filters, n_taps, n) == (C, K, M, N)
        spectra = _at(d_spectra, np.complex64, K * N).reshape(K, N)
        assert np.array_equal(spectra, fm.spectra(self.h, N, mode == "correlate").astype(np.complex64))
        rows = self.model_rows(_at(d_signal, self.bank.dtype, C * length).reshape(C, length), mode == "correlate")
        keep = np.ones(rows.shape, bool)
        if self.spoil is not None:
            self.spoil(rows, keep, d_output)
        out = _at(d_output, self.bank.dtype, rows.size).reshape(rows.shape)
        out[keep] = rows[keep]

    def run(self, mode, spoil=None, **kw):
        self.spoil = spoil
        try:
            return self.bank.run(self.x, self.h, N, mode, **kw)
        finally:
            self.spoil = None

    def direction(self, rng, shape):
        """rows of unit norm whose elements all have the same magnitude: a random phase, or a random sign in the real layout"""
        d = rng.integers(0, 2, shape) * 2.0 - 1.0 if self.real else np.exp(2j * np.pi * rng.random(shape))
        return d / np.sqrt(shape[-1])


@pytest.fixture(scope="module", params=("complex", "real"))
def layout(request):
    return Layout(request.param == "real")


@pytest.mark.parametrize("mode", gh.MODES)
def test_an_honest_bank_passes_the_run_and_the_row_check(layout, mode):
    got = layout.run(mode)
    assert got.shape == (C, K, L) and got.dtype == layout.bank.dtype
    assert np.array_equal(gh._bits(got), gh._bits(layout.model_rows(layout.x, mode == "correlate").astype(layout.bank.dtype)))
    gh._check_rows(got, gh._reference(layout.x, layout.h, mode == "correlate"), "honest", layout.x, layout.h)
    assert layout.bank.units(L, N, M) == (2 if layout.real else 3) and layout.bank.tiles(L, C, N, M) == 1


def test_the_prepared_spectra_are_the_banks(layout):
    got = layout.bank.prepared(layout.h, N, "correlate")
    assert got.shape == (K, N) and np.array_equal(got, fm.spectra(layout.h, N, True).astype(np.complex64))


def test_a_write_past_the_output_fails(layout):
    def past(rows, keep, d_output):
        _at(d_output, layout.bank.dtype, rows.size + 1)[-1] = 0
    with pytest.raises(AssertionError, match="wrote past its output"):
        layout.run("convolve", spoil=past)


def test_an_unwritten_last_output_fails(layout):
    def lazy(rows, keep, d_output):
        keep[-1, -1, -1] = False
    with pytest.raises(AssertionError, match="outputs left unwritten"):
        layout.run("convolve", spoil=lazy)
    got = layout.run("convolve", spoil=lazy, finite=False)
    assert np.isnan(got[-1, -1, -1]) and np.isfinite(got.reshape(-1)[:-1].view(np.float32)).all()


@pytest.mark.parametrize("mode", gh.MODES)
def test_rows_pass_within_the_bounds_and_fail_beyond_them(layout, mode):
    rng = np.random.default_rng(11)
    x, h = layout.x, layout.h
    want = gh._reference(x, h, mode == "correlate")
    hn = np.linalg.norm(h, axis=-1)[None, :]
    l2_scale = np.maximum(np.linalg.norm(want, axis=-1), hn * np.linalg.norm(x, axis=-1)[:, None])
    max_scale = np.maximum(np.abs(want).max(axis=-1), hn * np.abs(x).max(axis=-1)[:, None])
    d = layout.direction(rng, want.shape) * (gh.ROW_REL_L2 * l2_scale)[..., None]

    def moved(factor, delta):
        def spoil(rows, keep, d_output):
            rows += factor * delta
        return layout.run(mode, spoil=spoil)

    gh._check_rows(moved(0.25, d), want, "a quarter", x, h)
    with pytest.raises(AssertionError, match=r"twice row \(c=0, k=0\): relL2=") as failure:
        gh._check_rows(moved(2, d), want, "twice", x, h)
    assert 1.9 * gh.ROW_REL_L2 < float(re.search(r"relL2=(\S+)", str(failure.value)).group(1)) < 2.1 * gh.ROW_REL_L2
    # one output of the last row alone, against the max bound
    one = np.zeros(want.shape)
    one[-1, -1, L // 2] = gh.ROW_MAX * max_scale[-1, -1]
    gh._check_rows(moved(0.25, one), want, "a quarter", x, h)
    with pytest.raises(AssertionError, match=r"twice row \(c=%d, k=%d\): relL2=" % (C - 1, K - 1)) as failure:
        gh._check_rows(moved(2, one), want, "twice", x, h)
    assert 1.9 * gh.ROW_MAX < float(re.search(r"maxrel=(\S+)", str(failure.value)).group(1)) < 2.1 * gh.ROW_MAX

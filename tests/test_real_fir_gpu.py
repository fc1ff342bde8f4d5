"""The overlap-save FIR filter banks for real signals and real taps on an MI355X (smfft_fir_real_prepare / smfft_fir_real_launch,
smfft_amd.fir_real) against fp64 NumPy: both modes at every transform length over a grid of taps, channels, filters and signal lengths
(odd segment counts put a pair without a second segment into the middle of a workgroup tile); the filter-group split, uneven groups
included; the grid-stride loop past the grid cap; the prepared spectra and spectra from elsewhere; a caller's stream, the benchmark form
and fir(); 64-bit output offsets; three probes (exact scaling, a NaN sample, a NaN tap); guarded buffers at offset bases.

The reference is tests/fir_gpu_harness.py's _reference on the real arrays and the check its _check_rows with its bounds unchanged
(relL2 <= 1e-6, max <= 5e-6 per (channel, filter) row, with the denominators tests/test_fir_gpu.py derives): the transforms, the
product and their rounding are the complex bank's, run on two real segments at once.  Outputs are prefilled with 0xFF, so an unwritten
one shows as NaN, and are followed by a guard of 4096 floats."""
import numpy as np
import pytest

from tests.fir_gpu_harness import MODES, Bank, _bits, _check_rows, _reference      # (puts tools/ on the path)
from tests.guarded_region import Region

import fir_plan_model as fm  # noqa: E402
import fir_real_model as frm  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [256, 512, 1024, 2048, 4096]


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def fr():
    from smfft_amd import fir_real
    fir_real.lib()
    return fir_real


@pytest.fixture(scope="module")
def bank(sm, fr):
    return Bank.of_real(sm, fr)


def _rand(rng, shape):
    return rng.standard_normal(shape).astype(np.float32)


def test_reference_is_numpys_definition_on_real_arrays():
    rng = np.random.default_rng(1)
    x, h = _rand(rng, (2, 300)), _rand(rng, (3, 17))
    for corr in (False, True):
        want = fm.direct(x, h, corr)
        assert np.max(np.abs(_reference(x, h, corr) - want)) <= 1e-12 * np.max(np.abs(want))


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_filter_bank_matches_numpy(sm, fr, bank, N, mode):
    rng = np.random.default_rng(N + (mode == "correlate"))
    F = 4096 // N                                    # pairs per workgroup tile
    for M in (1, 17, N // 4 + 1, N - 1):
        V = N - M + 1
        # L < M; one segment (a pair without a partner); a pair and a lone segment; 2F + 1 segments per channel, the last one ragged:
        # F + 1 pairs, so with 3 channels an absent partner sits in mid-tile and tiles straddle channel boundaries
        for L in (max(1, M // 2), V, 2 * V + 1, (2 * F + 1) * V - 3):
            for C, K in ((1, 1), (3, 5), (3, 64)):
                x, h = _rand(rng, (C, L)), _rand(rng, (K, M))
                got = bank.run(x, h, N, mode)
                _check_rows(got, _reference(x, h, mode == "correlate"), f"N={N} {mode} M={M} L={L} C={C} K={K}", x, h)


# ---- the filter groups and the grid-stride loop -------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M", [(256, 65), (1024, 257), (4096, 1025)])
def test_filter_group_split_is_bit_exact(bank, N, M):
    """K = 200 on a signal of 20 workgroup tiles of pairs: the launch splits the filters into 100 groups of 2; every row equals the
    K = 1 launch of its filter to the bit"""
    bank.check_group_split(N, M, 2 * 20 * (4096 // N) * (N - M + 1) - 7, tiles=20, plan=(2, 100))


@pytest.mark.parametrize("N,P,K,plan", [
    (4096, 700, 7, (3, 3)),              # 3 groups of 3 filters asked and launched; the last holds one
    (4096, 450, 12, (3, 4)),             # 5 groups asked, group size 3: 4 grid rows
    (256, 699 * 16 + 5, 7, (3, 3)),
    (256, 449 * 16 + 7, 12, (3, 4)),
])
@pytest.mark.parametrize("mode", MODES)
def test_uneven_filter_groups(bank, N, P, K, plan, mode):
    """The uneven-group cases of tests/test_fir_gpu.py with L rescaled to pairs: M = N - 1 (V = 2) and P pairs -- S = 2 P - 1 segments,
    so the last pair has no partner, and L = 2 S - 1 leaves the last segment one output -- on 700 / 450 tiles: filter groups of the
    rule's size with a shorter last group, and a grid of fewer rows than the groups the rule asked for.  Every row equals the K = 1
    launch of its filter (the same spectrum) to the bit and is within bounds against fp64."""
    L = 2 * (2 * P - 1) - 1
    assert frm.Pairs(L, N, N - 1, False).pairs() == P
    bank.check_uneven_groups(N, L, K, plan, mode)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_grid_stride_loop_with_wrapped_prefetch(bank, N, mode):
    """M = N - 1 (V = 2 outputs per segment), C = 3, K = 3, P = 10240 F + 1 pairs per channel (F = 4096 / N per tile): about 2.5 x 12288
    tiles, so every workgroup runs two or three tiles and after its last filter prefetches the first filter's spectrum for its next
    tile.  S = 2 P - 1: the last pair of every channel has no partner; tiles straddle channel boundaries for N < 4096 and the last one
    is partial; L = 2 S - 1 leaves the last segment one output.  Every row against fp64."""
    bank.check_grid_stride_loop(N, mode)


# ---- spectra ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_prepared_spectra(sm, bank, N):
    """smfft_fir_real_prepare = fft(pad(g)) / N of the real taps within the per-FFT tolerances; a launch with NumPy-prepared spectra and
    a launch with the spectra smfft_fir_prepare makes of the taps cast to complex64 each pass the row check"""
    complex_bank = Bank.complex(sm)
    bank.check_prepared_spectra(N, elsewhere=lambda h, n, mode: complex_bank.prepared(h.astype(np.complex64), n, mode))


# ---- entry forms -----------------------------------------------------------------------------------------------------------------
def test_caller_stream(bank):
    """prepare and launch on a stream from hipStreamCreate, then hipStreamSynchronize"""
    bank.check_caller_stream([(1024, 257)], C=2, K=9, L=50000)


def test_benchmark_form_adds_to_the_timer(bank):
    bank.check_benchmark_form(N=512, M=100, K=3, L=20000)


def test_host_convenience(sm, fr):
    """fir(): 1-D and (C, L) inputs, float64 input, the default transform length, the (C, K, L) float32 result"""
    rng = np.random.default_rng(7)
    x = rng.standard_normal(5000)
    h = rng.standard_normal(65)
    x32, h32 = x.astype(np.float32), h.astype(np.float32)
    for mode in MODES:
        got = fr.fir(x, h, mode)
        assert got.shape == (1, 1, 5000) and got.dtype == np.float32
        _check_rows(got, _reference(x32[None], h32[None], mode == "correlate"), f"fir() {mode}", x32[None], h32[None])
    x2, h2 = _rand(rng, (2, 3000)), _rand(rng, (3, 33))
    got = fr.fir(x2, h2, fft_size=1024)
    assert got.shape == (2, 3, 3000) and got.dtype == np.float32
    _check_rows(got, _reference(x2, h2, False), "fir() (C, L)", x2, h2)


# ---- 64-bit offsets ----------------------------------------------------------------------------------------------------------------
def test_output_offsets_beyond_two_to_the_31(bank):
    """C = 1, K = 64, L = 2^25 + 1000: 2^31 + 64000 output floats (8 GiB); sampled windows of the last two filter rows against
    np.convolve / np.correlate on the matching input slice.  Row K - 1 crosses element 2^31 at n = 2^31 - (K - 1) L: one window
    straddles it, the last ones lie beyond it."""
    N, M, K, L = 1024, 257, 64, (1 << 25) + 1000
    rng = np.random.default_rng(5)
    x = rng.standard_normal((1, L), dtype=np.float32)
    h = _rand(rng, (K, M))
    bank.check_output_offsets(x, h, N)


# ---- probes --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_probe_exact_scaling(sm, fr, bank, N):
    """every channel scaled by a power of two of its own scales its outputs exactly: the channels do not mix, and nothing in the
    kernel depends on the magnitude of the data"""
    rng = np.random.default_rng(40 + N)
    M, C, K = N // 4 + 1, 3, 4
    L = 5 * (N - M + 1) - 3
    x, h = _rand(rng, (C, L)), _rand(rng, (K, M))
    exps = np.array([-9, 0, 14])
    scaled = np.ldexp(x, exps[:, None]).astype(np.float32)
    for mode in MODES:
        spectra = bank.prepared(h, N, mode)
        base = bank.run(x, h, N, mode, spectra=spectra)
        got = bank.run(scaled, h, N, mode, spectra=spectra)
        assert np.array_equal(_bits(got), _bits(np.ldexp(base, exps[:, None, None]).astype(np.float32))), (N, mode)


def _pairs_reading(pr, n):
    return [p for p in range(pr.pairs()) if pr.load_range(p)[0] <= n < pr.load_range(p)[1]]


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_probe_nan_sample(sm, fr, bank, N, mode):
    """A NaN at one sample of channel 1 of 3 makes NaN exactly the outputs of the pairs whose load range contains it (the footprint of
    tools/fir_real_model.py), for every filter and in that channel only; every other output is bit-identical to the clean run.  S = 5
    segments: pairs (0, 1), (2, 3) and a lone segment 4.  The NaN sits in the overlap of two pairs; in the lone last segment; and in
    the second segment of pair 0 only, which poisons segment 0's outputs too (the pair is the scope) and none of pair 1's."""
    corr = mode == "correlate"
    rng = np.random.default_rng(50 + N + corr)
    M, C, K = N // 4 + 1, 3, 3
    V = N - M + 1
    L = 5 * V - 3
    pr = frm.Pairs(L, N, M, corr)
    assert pr.w.segments() == 5 and pr.pairs() == 3 and not pr.present(2, 1)
    x, h = _rand(rng, (C, L)), _rand(rng, (K, M))
    spectra = bank.prepared(h, N, mode)
    clean = bank.run(x, h, N, mode, spectra=spectra)
    overlap = 2 * V if corr else 2 * V - 1               # the look-ahead of segment 1 / the history of segment 2
    second = V + M - 1 if corr else V                    # read by segment 1, not by segment 0, not by pair 1
    assert _pairs_reading(pr, overlap) == [0, 1] and _pairs_reading(pr, L - 1) == [2] and _pairs_reading(pr, second) == [0]
    a0 = pr.load_start(0, 0)
    assert not (a0 <= second < a0 + N) and pr.load_start(0, 1) <= second < pr.load_start(0, 1) + N
    for n, hit_outputs in ((overlap, (0, 4 * V)), (L - 1, (4 * V, L)), (second, (0, 2 * V))):
        foot = frm.nan_footprint(L, N, M, corr, n)
        assert foot[hit_outputs[0]:hit_outputs[1]].all() and foot.sum() == hit_outputs[1] - hit_outputs[0]
        bad = x.copy()
        bad[1, n] = np.nan
        got = bank.run(bad, h, N, mode, spectra=spectra, finite=False)
        for k in range(K):
            assert np.array_equal(np.isnan(got[1, k]), foot), (N, mode, n, k)
            assert np.array_equal(_bits(got[1, k][~foot]), _bits(clean[1, k][~foot])), (N, mode, n, k)
        assert np.array_equal(_bits(got[[0, 2]]), _bits(clean[[0, 2]])), (N, mode, n)


@pytest.mark.parametrize("N", SIZES)
def test_probe_nan_tap(sm, fr, bank, N):
    """a NaN tap of one filter reaches exactly that filter's spectrum and rows, in every channel; the others are bit-identical"""
    rng = np.random.default_rng(60 + N)
    M, C, K = 17, 2, 5
    L = 3 * (N - M + 1) + 5
    x, h = _rand(rng, (C, L)), _rand(rng, (K, M))
    bad = h.copy()
    bad[3, 5] = np.nan
    for mode in MODES:
        spectra, bad_spectra = bank.prepared(h, N, mode), bank.prepared(bad, N, mode)
        others = [0, 1, 2, 4]
        assert np.isnan(bad_spectra[3]).all()            # every element, in a part at least: real taps keep some imaginary parts +0
        assert np.array_equal(bad_spectra[others].view(np.uint32), spectra[others].view(np.uint32))
        clean = bank.run(x, h, N, mode, spectra=spectra)
        got = bank.run(x, bad, N, mode, spectra=bad_spectra, finite=False)
        assert np.isnan(got[:, 3]).all(), (N, mode)
        assert np.array_equal(_bits(got[:, others]), _bits(clean[:, others])), (N, mode)


# ---- bounds ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_bounds(sm, fr, bank, N, mode):
    """prepare and launch separately, every buffer a guarded allocation of its own whose payload ends where the NaN guard begins, at
    offset bases (signal and output at an odd float, taps at a float of their own, spectra at an odd float2): the guard in front of
    channel 0 is what a convolution's history would read, the one behind channel C - 1 what a correlation's look-ahead -- or a
    partner that is not there -- would read; both must come in as zeros, never as NaN.  Nothing outside spectra[0, K N) and
    out[0, C K L) changes, and the result does not depend on the placement."""
    corr = 1 if mode == "correlate" else 0
    rng = np.random.default_rng(70 + N + corr)
    for M in (1, N // 4 + 1, N - 1):
        V = N - M + 1
        for L in (max(1, M - 1), V, 3 * V + V // 3 + 1):
            for C, K in ((1, 1), (3, 5)):
                x, h = _rand(rng, (C, L)), _rand(rng, (K, M))
                what = f"N={N} {mode} M={M} L={L} C={C} K={K}"
                sig, taps = Region(sm, x.view(np.uint8).reshape(-1), 4, align=4), Region(sm, h.view(np.uint8).reshape(-1), 12, align=4)
                spec = Region(sm, np.full(K * N * 8, 0xFF, np.uint8), 8)
                out = Region(sm, np.full(C * K * L * 4, 0xFF, np.uint8), 20, align=4)
                try:
                    assert fr.lib().smfft_fir_real_prepare(taps.ptr, M, K, N, corr, spec.ptr, None) == 0
                    assert sm.lib.smfft_synchronize() == 0
                    spectra = spec.outside_unchanged(False).view(np.complex64).reshape(K, N)
                    for r in (sig, taps, out):
                        r.outside_unchanged(True)
                    assert np.array_equal(spectra.view(np.uint32), bank.prepared(h, N, mode).view(np.uint32)), f"{what}: spectra depend on placement"
                    spec.image[spec.lo:spec.lo + spec.n] = spectra.view(np.uint8).reshape(-1)
                    assert fr.lib().smfft_fir_real_launch(sig.ptr, L, C, spec.ptr, K, M, N, corr, out.ptr, None) == 0
                    assert sm.lib.smfft_synchronize() == 0
                    got = out.outside_unchanged(False).view(np.float32).reshape(C, K, L)
                    for r in (sig, taps, spec):
                        r.outside_unchanged(True)
                finally:
                    for r in (sig, taps, spec, out):
                        r.buf.free()
                assert np.all(np.isfinite(got)), f"{what}: a guard was read, or an output left unwritten"
                _check_rows(got, _reference(x, h, bool(corr)), what, x, h)
                assert np.array_equal(_bits(got), _bits(fr.fir(x, h, mode, fft_size=N))), f"{what}: result depends on placement"

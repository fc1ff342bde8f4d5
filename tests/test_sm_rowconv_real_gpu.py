"""The real row-pair convolutions on an MI355X (smfft_rowconv_real_launch, smfft_amd.rowconv_real; one kernel per inner length
M = 256 ... 4096) against the sum of the definition in fp64 (tools/rowconv_real_model.py `direct`): Gaussian row pairs on both sides of
every M boundary, with n_a and with n_b above M / 2, in both modes; rows whose scales differ by up to 2^60, which the kernel's balancing
of the two packed rows must carry to the bit; exact probes (impulses, the autocorrelation of one buffer, NaN, Inf and zero rows); the
place of a row pair in its batch, which must not show in the bits; windows, which must be slices of the full result to the bit; the
grid size, which must not show either; the grid-stride loop; guarded buffers at interior and odd bases; 64-bit offsets on either input
side and on the output side; a caller's stream, the benchmark form and the host round trip.

Every run goes into an output prefilled with 0xFF (NaN), with a guard of 4096 elements of 0x5A on both sides that must stay untouched;
inputs end where their allocation ends.  Elements are float32: 4 bytes.

The bound for full outputs, per row against fp64: ||d||_2 / ||want||_2 <= ROW_REL_L2 and max |d| / max |want| <= ROW_MAX, the FIR
bank's bounds (tests/fir_gpu_harness.py), which tests/test_sm_rowconv_gpu.py holds the complex kernel to: the project's bound for this
chain.  An fp32 NumPy model of the chain (tools/rowconv_real_model.py `model` with float32) gave relL2 <= 1.4e-7 and
max |d| / max |want| <= 2.1e-7 over all shapes below and b scaled by 2^-60 ... 2^60 (tests/test_sm_rowconv_real_cpu.py), so the bound is
seven times the model's worst figure; full Gaussian rows are well conditioned and none is drawn again.  Windowed outputs are not judged
by a relative bound -- a narrow window can lie where the row's outputs are small -- but must equal the same elements of the full
launch to the bit.  The one exception is the two m = 1 cases of the 64-bit offset test, where a full launch would need 8 GiB twice
over: there the bound is the row bound on the one output, and a row pair is drawn again while that output is below half its
expectation, |want| < ||full want||_2 / (2 sqrt(Lfull)), judged from the fp64 reference alone and never from the kernel's output (the
error of the chain scales with the whole row, so it is relative to one output only where that output is of the row's size).  The tests
print the worst figures they measure per M.

The file's name makes it collect behind every older GPU test file, so that each of those keeps its place in a run of the suite."""
import ctypes
import os
import sys

import numpy as np
import pytest

from tests import rows_gpu_harness as rh
from tests.fir_gpu_harness import GRID_CAP, GUARD, ROW_MAX, ROW_REL_L2

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import rowconv_real_model as rrm  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [256, 512, 1024, 2048, 4096]
LARGEST = {256: (128, 129), 512: (256, 257), 1024: (512, 513), 2048: (1024, 1025), 4096: (2048, 2049)}      # n_a + n_b - 1 = M
MODES = (False, True)       # correlate
SCALES = (-60, -12, -1, 0, 1, 12, 60)
WORST = rh.Worst()      # M -> [relL2, max / max]: the worst figures measured in this run
E = 4                       # bytes per element


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def rc():
    from smfft_amd import rowconv_real
    rowconv_real.lib()
    return rowconv_real


def _mode(correlate):
    return "correlate" if correlate else "convolve"


def _check_rows(got, want, M, what):
    """got, want: (batch, m); prints the worst row figures before it asserts"""
    d = got.astype(np.float64) - want
    l2 = np.linalg.norm(d, axis=1) / np.maximum(np.linalg.norm(want, axis=1), 1e-300)
    mx = np.max(np.abs(d), axis=1) / np.maximum(np.max(np.abs(want), axis=1), 1e-300)
    worst = WORST.record(M, l2, mx)
    print(f"{what}: worst row relL2 = {l2.max():.3e}, max |d| / max |want| = {mx.max():.3e}  (M = {M} so far: {worst[0]:.3e}, {worst[1]:.3e})")
    assert l2.max() <= ROW_REL_L2 and mx.max() <= ROW_MAX, f"{what}: row {int(np.argmax(l2))} relL2 = {l2.max():.3e}, row {int(np.argmax(mx))} max = {mx.max():.3e}"


def run(sm, rc, a, b, correlate, first=0, m=None, front=0, finite=True, launch=None):
    """one launch through the device-pointer API on copies of a = (batch, n_a) and b = (batch, n_b) float32 that end where their
    allocations end; b = None: d_b = d_a, one buffer for both.  Returns the (batch, m) result after checking the guards and (finite)
    that no NaN of the prefill is left.  m = None: the full result behind `first`.  front: elements between the output's front guard
    and the output's base; launch(da, db, dout, n_a, n_b, first, m, batch, correlate): how to launch, when not on the null stream
    through the mirror"""
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32 and a.ndim == 2
    batch, n_a = a.shape
    da = rh.upload(sm, a)
    if b is None:
        db, pb, n_b = None, da.ptr, n_a
    else:
        b = np.ascontiguousarray(b)
        assert b.dtype == np.float32 and b.shape[0] == batch
        n_b = b.shape[1]
        db = rh.upload(sm, b)
        pb = db.ptr
    first, m = rrm.window(n_a, n_b, first, m)
    dout, pout = rh.guarded(sm, batch * m, E, front)
    try:
        if launch is None:
            rc.launch(da.ptr, pb, pout, n_a, n_b, first, m, batch, correlate)
        else:
            launch(da.ptr, pb, pout, n_a, n_b, first, m, batch, correlate)
        assert sm.lib.smfft_synchronize() == 0
        return rh.collect(dout, batch * m, np.float32, front, finite).reshape(batch, m)
    finally:
        for buf in (da, db, dout):
            if buf is not None:
                buf.free()


def _ffts(n_a, n_b):
    return 4096 // rrm.fft_size(n_a, n_b)


def _batch(n_a, n_b, tiles=2, extra=1):
    return tiles * _ffts(n_a, n_b) + extra


# ---- 1: fp64 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_a, n_b", [(1, 1), (1, 256), (256, 1), (128, 129), (129, 129),            # M boundaries, degenerate rows
                                      (300, 200), (200, 300),                                          # n_a > M / 2, n_b > M / 2
                                      (1000, 25), (1000, 26),                                          # the 1024 / 2048 boundary
                                      (4095, 2), (2, 4095),                                            # a thread's last element, on either side
                                      (4096, 1), (1, 4096), (2048, 2049),                              # energies 2^12 apart; the largest
                                      (1536, 513)])                                                    # asymmetric and large
def test_against_fp64(sm, rc, n_a, n_b):
    """batch = 2F + 1 (two full tiles and one row), the full output, both modes"""
    rng = np.random.default_rng(1000 * n_a + n_b)
    batch = _batch(n_a, n_b)
    a, b = rh.rand(rng, (batch, n_a)), rh.rand(rng, (batch, n_b))
    for correlate in MODES:
        got = run(sm, rc, a, b, correlate)
        assert got.shape == (batch, n_a + n_b - 1) and got.dtype == np.float32
        _check_rows(got, rrm.direct(a, b, correlate), rrm.fft_size(n_a, n_b), f"n_a={n_a} n_b={n_b} {_mode(correlate)}")


@pytest.mark.parametrize("n_a, n_b", [(300, 200), (2048, 2049)])
def test_scales(sm, rc, n_a, n_b):
    """b[r] multiplied by 2^s, s cycling per row through -60, -12, -1, 0, 1, 12, 60 (batch = 2F + 1, at least one row per scale), both
    modes: the row bounds hold against the fp64 sum of the scaled rows, and ldexp(got, -s) equals the unscaled run to the bit -- the
    kernel's scales are exact powers of two chosen per row.  The chain without the balancing cannot pass either half"""
    rng = np.random.default_rng(30 + n_a)
    batch = max(_batch(n_a, n_b), len(SCALES))
    a, b = rh.rand(rng, (batch, n_a)), rh.rand(rng, (batch, n_b))
    s = np.array([SCALES[r % len(SCALES)] for r in range(batch)], np.int32)
    scaled = np.ldexp(b, s[:, None]).astype(np.float32)
    assert np.array_equal(np.ldexp(scaled, -s[:, None]).astype(np.float32), b)          # exact: nothing left the normal range
    for correlate in MODES:
        base = run(sm, rc, a, b, correlate)
        got = run(sm, rc, a, scaled, correlate)
        _check_rows(got, rrm.direct(a, scaled, correlate), rrm.fft_size(n_a, n_b), f"n_a={n_a} n_b={n_b} {_mode(correlate)} b * 2^s")
        back = np.ldexp(got, -s[:, None]).astype(np.float32)
        differ = np.flatnonzero((rh.bits(back) != rh.bits(base)).any(axis=1))
        print(f"n_a={n_a} n_b={n_b} {_mode(correlate)}: {differ.size} of {batch} rows differ from the unscaled run after ldexp(-s)")
        assert differ.size == 0, (n_a, n_b, correlate, [(int(r), int(s[r])) for r in differ])


# ---- 2: exact probes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_a, n_b", [(300, 200), (128, 129), (1000, 25), (2048, 2049), (1536, 513)])
def test_probe_impulses(sm, rc, n_a, n_b):
    """row r of a = a unit impulse at j0 in {0, 1, n_a / 2, n_a - 1}, b Gaussian: the output is b (convolve) or b reversed (correlate) at
    j0 ... j0 + n_b - 1 and zero elsewhere, every element within ROW_MAX max |b|"""
    js = sorted({0, 1, n_a // 2, n_a - 1})
    rng = np.random.default_rng(40 + n_a)
    a = np.zeros((len(js), n_a), np.float32)
    a[np.arange(len(js)), js] = 1
    b = rh.rand(rng, (len(js), n_b))
    for correlate in MODES:
        got = run(sm, rc, a, b, correlate).astype(np.float64)
        second = rrm.second_operand(b.astype(np.float64), correlate)
        for r, j0 in enumerate(js):
            want = np.zeros(n_a + n_b - 1, np.float64)
            want[j0:j0 + n_b] = second[r]
            err, scale = np.max(np.abs(got[r] - want)), np.max(np.abs(b[r]))
            print(f"n_a={n_a} n_b={n_b} {_mode(correlate)} impulse at {j0}: max |d| / max |b| = {err / scale:.3e}")
            assert err <= ROW_MAX * scale, (n_a, n_b, correlate, j0, err / scale)


@pytest.mark.parametrize("n", [129, 2048])
def test_probe_autocorrelation(sm, rc, n):
    """d_a == d_b with correlate set, batch = 2F + 1: the fp64 autocorrelation within the row bounds; lag 0, at index n - 1, is ||a||^2
    within ROW_MAX ||a||^2; the result is even in the lag, |y[k] - y[2n - 2 - k]| <= ROW_MAX ||a||^2; and the bits are those of two
    buffers with the same content"""
    rng = np.random.default_rng(45 + n)
    a = rh.rand(rng, (_batch(n, n), n))
    got = run(sm, rc, a, None, True)
    assert got.shape == (a.shape[0], 2 * n - 1)
    _check_rows(got, rrm.direct(a, a, True), rrm.fft_size(n, n), f"autocorrelation n={n}")
    energy = np.sum(a.astype(np.float64) ** 2, axis=1)
    err = np.abs(got[:, n - 1].astype(np.float64) - energy) / energy
    odd = np.max(np.abs(got.astype(np.float64) - got[:, ::-1].astype(np.float64)), axis=1) / energy
    print(f"autocorrelation n={n}: worst |y[n - 1] - ||a||^2| / ||a||^2 = {err.max():.3e}, worst |y[k] - y[2n - 2 - k]| / ||a||^2 = {odd.max():.3e}")
    assert err.max() <= ROW_MAX and odd.max() <= ROW_MAX, (n, err.max(), odd.max())
    assert np.array_equal(rh.bits(got), rh.bits(run(sm, rc, a, a.copy(), True))), n


# ---- 3: the window ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_a, n_b", [(300, 200), (2048, 2049), (1, 4096)])
def test_window(sm, rc, n_a, n_b):
    """(first, m) in {(0, 1), (Lfull - 1, 1), (n_b - 1 - 3, 7) where it fits (the lags -3 ... 3), (1, Lfull - 2)}, batch = 2F + 1, both
    modes: the bits of the slice of the full run, which passes the fp64 bound; the guards on both sides of the batch * m outputs stay.
    With m odd the rows' bases are odd element offsets, which 4-byte rows allow"""
    full = n_a + n_b - 1
    windows = [(0, 1), (full - 1, 1), (1, full - 2)] + ([(n_b - 4, 7)] if n_b - 4 >= 0 and n_b + 3 <= full else [])
    assert (len(windows) == 3) == ((n_a, n_b) == (1, 4096))
    rng = np.random.default_rng(55 + n_a)
    batch = _batch(n_a, n_b)
    a, b = rh.rand(rng, (batch, n_a)), rh.rand(rng, (batch, n_b))
    for correlate in MODES:
        base = run(sm, rc, a, b, correlate)
        _check_rows(base, rrm.direct(a, b, correlate), rrm.fft_size(n_a, n_b), f"n_a={n_a} n_b={n_b} {_mode(correlate)} full")
        for first, m in windows:
            got = run(sm, rc, a, b, correlate, first=first, m=m)
            assert got.shape == (batch, m)
            assert np.array_equal(rh.bits(got), rh.bits(base[:, first:first + m])), (n_a, n_b, correlate, first, m)


# ---- 4: isolation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_a, n_b", [(128, 129), (300, 200), (2048, 2049)])
def test_probe_rows_are_isolated(sm, rc, n_a, n_b):
    """batch = 3F, four runs per mode: one row of a all NaN; one row of b with a single NaN sample; one row of a all zero; one row of a
    with a single +Inf sample.  The poisoned row is NaN in all its outputs, the zero row's are +0 bits, and every other row keeps the
    bits of the clean run"""
    F = _ffts(n_a, n_b)
    rng = np.random.default_rng(50 + n_a)
    a, b = rh.rand(rng, (3 * F, n_a)), rh.rand(rng, (3 * F, n_b))
    whole, single, zero, inf = F + F // 2, 2 * F + F // 3, F // 5, 2 * F + F // 2
    assert len({whole, single, zero}) == 3 and inf < 3 * F
    for correlate in MODES:
        clean = run(sm, rc, a, b, correlate)
        _check_rows(clean, rrm.direct(a, b, correlate), rrm.fft_size(n_a, n_b), f"n_a={n_a} n_b={n_b} {_mode(correlate)} clean")
        for case, row in (("a all NaN", whole), ("b one NaN", single), ("a all zero", zero), ("a one +Inf", inf)):
            bad_a, bad_b = a.copy(), b.copy()
            if case == "a all NaN":
                bad_a[row] = np.nan
            elif case == "b one NaN":
                bad_b[row, n_b // 3] = np.nan
            elif case == "a one +Inf":
                bad_a[row, n_a // 2] = np.inf
            else:
                bad_a[row] = 0
            got = run(sm, rc, bad_a, bad_b, correlate, finite=False)
            assert got.shape == clean.shape
            if case == "a all zero":
                words = rh.bits(got[row])
                print(f"n_a={n_a} n_b={n_b} {_mode(correlate)} zero row: {int(np.count_nonzero(words))} words that are not +0")
                assert not words.any(), (n_a, n_b, correlate, "a zero row is not +0 everywhere")
            else:
                assert np.isnan(got[row]).all(), (n_a, n_b, correlate, case, int(np.isnan(got[row]).sum()))
            others = np.arange(3 * F) != row
            assert np.array_equal(rh.bits(got[others]), rh.bits(clean[others])), (n_a, n_b, correlate, case)


@pytest.mark.parametrize("M", [256, 1024, 4096])
def test_row_bits_do_not_depend_on_position(sm, rc, M):
    """the largest shape of M, both modes: one pair at row 0 and at row F - 1 of a batch of 2F + 1, alone in a batch of 1, and as the
    last row of a ragged tile (batch F + 2, or 2 where F = 1) among other Gaussian rows of differing scales: the same bits in all four
    placements -- the reductions behind the row's exponent see the row's own threads only, in one order"""
    n_a, n_b = LARGEST[M]
    F = 4096 // M
    rng = np.random.default_rng(80 + M)
    pa, pb = rh.rand(rng, (1, n_a)), np.ldexp(rh.rand(rng, (1, n_b)), 5).astype(np.float32)
    for correlate in MODES:
        alone = run(sm, rc, pa, pb, correlate)
        _check_rows(alone, rrm.direct(pa, pb, correlate), M, f"M={M} {_mode(correlate)} alone")
        for batch, row in ((2 * F + 1, 0), (2 * F + 1, F - 1), (F + 2, F + 1)):
            a = np.ldexp(rh.rand(rng, (batch, n_a)), rng.integers(-20, 20, (batch, 1))).astype(np.float32)
            b = np.ldexp(rh.rand(rng, (batch, n_b)), rng.integers(-20, 20, (batch, 1))).astype(np.float32)
            a[row], b[row] = pa[0], pb[0]
            got = run(sm, rc, a, b, correlate)
            assert np.array_equal(rh.bits(got[row]), rh.bits(alone[0])), (M, correlate, batch, row)


# ---- 5: the grid --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", SIZES)
def test_grid_is_invisible(sm, rc, M):
    """the largest shape of M (Lfull = M), batch = 5F + 1 (six tiles), both modes: launch_tuned on 1, 2, 3, 6 and 12288 workgroups gives
    the bits of launch.  One workgroup runs all six tiles"""
    n_a, n_b = LARGEST[M]
    assert rrm.fft_size(n_a, n_b) == M and n_a + n_b - 1 == M
    rng = np.random.default_rng(60 + M)
    batch = _batch(n_a, n_b, 5)
    a, b = rh.rand(rng, (batch, n_a)), rh.rand(rng, (batch, n_b))
    for correlate in MODES:
        base = run(sm, rc, a, b, correlate)
        _check_rows(base, rrm.direct(a, b, correlate), M, f"M={M} n_a={n_a} n_b={n_b} {_mode(correlate)} six tiles")
        for grid in (1, 2, 3, 6, 12288):
            got = run(sm, rc, a, b, correlate, launch=lambda da, db, dout, na, nb, first, m, bt, c: rc.launch_tuned(da, db, dout, na, nb, first, m, bt, grid, c))
            assert np.array_equal(rh.bits(got), rh.bits(base)), (M, correlate, grid)


@pytest.mark.parametrize("n_a, n_b, batch, correlate", [(5, 3, 16 * (2 * 12288) + 7, False), (1025, 1024, 2 * 12288 + 1, True)])
def test_grid_stride_loop(sm, rc, n_a, n_b, batch, correlate):
    """more tiles than the grid cap through the plain launch: at (5, 3), M = 256, every workgroup runs two or three tiles of sixteen
    rows; at (1025, 1024), M = 2048, one workgroup runs a second tile, the partial last one.  Every row against fp64: at (5, 3) the
    sum itself; at (1025, 1024), where the sum over 24577 rows would take a minute, the fp64 chain (rrm.model in float64, which
    tests/test_sm_rowconv_real_cpu.py holds within 1e-12 of `direct`) and the rows of the first, the wrapping and the last tiles
    against the sum"""
    F = _ffts(n_a, n_b)
    assert GRID_CAP == 12288 and GRID_CAP < -(-batch // F) <= 3 * GRID_CAP and batch % F
    rng = np.random.default_rng(12288 + n_a)
    a, b = rh.rand(rng, (batch, n_a)), rh.rand(rng, (batch, n_b))
    got = run(sm, rc, a, b, correlate)
    M = rrm.fft_size(n_a, n_b)
    what = f"grid-stride n_a={n_a} n_b={n_b} batch={batch} {_mode(correlate)}"
    if min(n_a, n_b) <= 16:
        _check_rows(got, rrm.direct(a, b, correlate), M, what)
    else:
        _check_rows(got, rrm.model(a, b, correlate), M, what + ", fp64 chain")
        rows = sorted({0, F - 1, GRID_CAP * F - 1, GRID_CAP * F, 2 * GRID_CAP * F - 1, 2 * GRID_CAP * F, batch - 1} & set(range(batch)))
        _check_rows(got[rows], rrm.direct(a[rows], b[rows], correlate), M, what + f", rows {rows}, the sum")


# ---- 6: bounds and placement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_a, n_b, correlate", [(300, 200, True), (1, 4096, False), (4096, 1, True)])
def test_bounds(sm, rc, n_a, n_b, correlate):
    """batch in {1, F - 1, F + 1}, the inputs ending where their allocations end, the output base 1 and 3 elements behind its front
    guard: nothing in front of or behind the output changes, every output is written, and the bits are those at the aligned base,
    which pass the fp64 bound; so are those of the lag-0 window alone, at an odd base"""
    F = _ffts(n_a, n_b)
    rng = np.random.default_rng(70 + n_a)
    for batch in sorted({1, F + 1} | ({F - 1} if F > 1 else set())):
        a, b = rh.rand(rng, (batch, n_a)), rh.rand(rng, (batch, n_b))
        base = run(sm, rc, a, b, correlate)
        _check_rows(base, rrm.direct(a, b, correlate), rrm.fft_size(n_a, n_b), f"n_a={n_a} n_b={n_b} batch={batch}")
        for front in (1, 3):
            got = run(sm, rc, a, b, correlate, front=front)
            assert np.array_equal(rh.bits(got), rh.bits(base)), f"n_a={n_a} n_b={n_b} batch={batch} front={front}: the result depends on placement"
            window = run(sm, rc, a, b, correlate, first=n_b - 1, m=1, front=front)            # lag 0 alone, at an odd base
            assert np.array_equal(rh.bits(window), rh.bits(base[:, n_b - 1:n_b])), (n_a, n_b, batch, front)


# ---- 7: 64-bit offsets ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_a, n_b, first, m, correlate", [(4095, 2, 2047, 1, False), (2, 4095, 2047, 1, True), (2048, 2048, 0, 4095, True)])
def test_offsets_beyond_two_to_the_31(sm, rc, n_a, n_b, first, m, correlate):
    """batch = ceil(2^31 / 4095) + 8 rows: 8 GiB of a (n_a = 4095), of b (n_b = 4095, read backwards in correlate mode) or of output
    (m = 4095).  The inputs are memset to zero, with Gaussian rows at row 0, at the row that straddles element 2^31 of the large side
    and at the last two rows: those rows pass the bound (the m = 1 rows drawn well conditioned, see the head of the file), zero rows
    give exactly +0 (all of them where m = 1, sampled ones where the output is the large side), every one of them was written over the
    0xFF prefill, and the guard behind the output is intact"""
    big = max(n_a, n_b, m)
    assert big == 4095
    batch = -(-(1 << 31) // big) + 8
    straddle = (1 << 31) // big
    assert straddle * big < (1 << 31) < (straddle + 1) * big and (batch - 2) * big > (1 << 31)
    rows = [0, straddle, batch - 2, batch - 1]
    zeros = [1, straddle // 2, straddle - 1, straddle + 1, batch - 3]
    full = n_a + n_b - 1
    rng = np.random.default_rng(31 + n_a)
    a, b = rh.rand(rng, (len(rows), n_a)), rh.rand(rng, (len(rows), n_b))
    want_full = rrm.direct(a, b, correlate)
    while m < full:       # (m = 1: a pair whose one output is below half its expectation is drawn again)
        small = np.linalg.norm(want_full[:, first:first + m], axis=1) < 0.5 * np.sqrt(m / full) * np.linalg.norm(want_full, axis=1)
        if not small.any():
            break
        a[small], b[small] = rh.rand(rng, (int(small.sum()), n_a)), rh.rand(rng, (int(small.sum()), n_b))
        want_full = rrm.direct(a, b, correlate)
    want = want_full[:, first:first + m]
    da, db = sm.DeviceBuffer(batch * n_a * E), sm.DeviceBuffer(batch * n_b * E)
    dout = sm.DeviceBuffer((batch * m + GUARD) * E)
    try:
        assert sm.lib.smfft_memset(da.ptr, 0, batch * n_a * E) == 0
        assert sm.lib.smfft_memset(db.ptr, 0, batch * n_b * E) == 0
        assert sm.lib.smfft_memset(dout.ptr, 0xFF, batch * m * E) == 0
        assert sm.lib.smfft_memset(dout.ptr + batch * m * E, 0x5A, GUARD * E) == 0
        for i, r in enumerate(rows):
            assert sm.lib.smfft_memcpy_h2d(da.ptr + r * n_a * E, a[i].ctypes.data, n_a * E) == 0
            assert sm.lib.smfft_memcpy_h2d(db.ptr + r * n_b * E, b[i].ctypes.data, n_b * E) == 0
        rc.launch(da.ptr, db.ptr, dout.ptr, n_a, n_b, first, m, batch, correlate)
        assert sm.lib.smfft_synchronize() == 0
        guard = np.empty(GUARD, np.uint32)
        assert sm.lib.smfft_memcpy_d2h(guard.ctypes.data, dout.ptr + batch * m * E, guard.nbytes) == 0
        assert np.all(guard == 0x5A5A5A5A), "the kernel wrote past its output"
        got = np.empty((len(rows), m), np.float32)
        for i, r in enumerate(rows):
            assert sm.lib.smfft_memcpy_d2h(got[i].ctypes.data, dout.ptr + r * m * E, m * E) == 0
        _check_rows(got, want, 4096, f"2^31 rows n_a={n_a} n_b={n_b} first={first} m={m} {_mode(correlate)}")
        if m == 1:
            whole = np.empty(batch, np.float32)
            assert sm.lib.smfft_memcpy_d2h(whole.ctypes.data, dout.ptr, whole.nbytes) == 0
            words = rh.bits(np.delete(whole, rows))
            print(f"{words.size} zero rows: {int(np.count_nonzero(words))} words that are not +0")
            assert not words.any(), "a zero row is not +0"
        else:
            for r in zeros:
                row = np.empty(m, np.float32)
                assert sm.lib.smfft_memcpy_d2h(row.ctypes.data, dout.ptr + r * m * E, m * E) == 0
                words = rh.bits(row)
                print(f"zero row {r}: {int(np.count_nonzero(words))} words that are not +0 ({int(np.count_nonzero(words == 0x80000000))} of them -0)")
                assert not words.any(), f"zero row {r} is not +0 everywhere"
    finally:
        for buf in (da, db, dout):
            buf.free()


# ---- 8: entry forms ---------------------------------------------------------------------------------------------------------------------
def test_caller_stream(sm, rc):
    """launch on a stream from hipStreamCreate, then hipStreamSynchronize"""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value
    rng = np.random.default_rng(11)
    for n_a, n_b, correlate in ((1000, 25, True), (100, 300, False)):
        a, b = rh.rand(rng, (37, n_a)), rh.rand(rng, (37, n_b))

        def launch(da, db, dout, na, nb, first, m, batch, c):
            assert sm.lib.smfft_synchronize() == 0                              # the prefill of the output, on the null stream
            rc.launch(da, db, dout, na, nb, first, m, batch, c, stream=stream.value)
            assert hip.hipStreamSynchronize(stream) == 0
        _check_rows(run(sm, rc, a, b, correlate, launch=launch), rrm.direct(a, b, correlate), rrm.fft_size(n_a, n_b), f"stream n_a={n_a} n_b={n_b}")
    assert hip.hipStreamDestroy(stream) == 0


def test_benchmark_form_adds_to_the_timer(sm, rc):
    """the library's smfft_rowconv_real_benchmark adds its milliseconds to a non-zero total and fills the output; so does the mirror's"""
    n_a, n_b = 1536, 513
    rng = np.random.default_rng(12)
    a, b = rh.rand(rng, (300, n_a)), rh.rand(rng, (300, n_b))
    total = ctypes.c_double(1.0)

    def c_form(da, db, dout, na, nb, first, m, batch, c):
        assert rc.lib().smfft_rowconv_real_benchmark(da, db, dout, na, nb, first, m, batch, int(c), ctypes.byref(total)) == 0
        assert total.value > 1.0
    out = run(sm, rc, a, b, True, launch=c_form)
    _check_rows(out, rrm.direct(a, b, True), 2048, "benchmark form")

    def mirror(da, db, dout, na, nb, first, m, batch, c):
        status, ms = rc.benchmark(da, db, dout, na, nb, first, m, batch, c)
        assert status == 0 and ms > 0.0
    assert np.array_equal(rh.bits(run(sm, rc, a, b, True, launch=mirror)), rh.bits(out))


def test_host_round_trip(sm, rc):
    """rowconv_real.convolve on 1-D, 3-D and float64 inputs against np.convolve and np.correlate: float32 of shape (..., m), the bits of
    the device-pointer launch; a +-16-lag window and the tail window are slices; an empty batch returns an empty array; complex input
    raises TypeError"""
    rng = np.random.default_rng(7)
    a1, b1 = rng.standard_normal(1000), rng.standard_normal(25)                      # 1-D float64
    a32, b32 = a1.astype(np.float32), b1.astype(np.float32)
    got = rc.convolve(a1, b1)
    assert got.shape == (1024,) and got.dtype == np.float32
    assert np.array_equal(rh.bits(got), rh.bits(run(sm, rc, a32[None], b32[None], False)[0]))
    _check_rows(got[None], np.convolve(a32.astype(np.float64), b32.astype(np.float64))[None], 1024, "convolve() 1-D against np.convolve")
    got = rc.convolve(a1, b1, correlate=True)
    _check_rows(got[None], np.correlate(a32.astype(np.float64), b32.astype(np.float64), "full")[None], 1024, "convolve() 1-D against np.correlate")
    lags = rc.convolve(a1, b1, correlate=True, first=25 - 1 - 16, m=33)              # the lags -16 ... 16
    assert lags.shape == (33,) and np.array_equal(rh.bits(lags), rh.bits(got[8:41]))
    tail = rc.convolve(a1, b1, first=1000)
    assert tail.shape == (24,) and np.array_equal(rh.bits(tail), rh.bits(rc.convolve(a1, b1)[1000:]))
    a3, b3 = rh.rand(rng, (2, 3, 257)), rh.rand(rng, (2, 3, 100))
    got = rc.convolve(a3, b3, correlate=True)
    assert got.shape == (2, 3, 356) and got.dtype == np.float32
    assert np.array_equal(rh.bits(got.reshape(6, 356)), rh.bits(run(sm, rc, a3.reshape(6, 257), b3.reshape(6, 100), True)))
    want = np.stack([np.correlate(a3.reshape(6, 257)[r].astype(np.float64), b3.reshape(6, 100)[r].astype(np.float64), "full") for r in range(6)])
    _check_rows(got.reshape(6, 356), want, 512, "convolve() 3-D against np.correlate")
    empty = rc.convolve(np.zeros((0, 5), np.float32), np.zeros((0, 3), np.float32))
    assert empty.shape == (0, 7) and empty.dtype == np.float32
    with pytest.raises(TypeError):
        rc.convolve(a1.astype(np.complex64), b1)
    assert ROW_REL_L2 == 1e-6 and ROW_MAX == 5e-6

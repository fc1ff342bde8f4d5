"""The row-pair convolutions on an MI355X (smfft_rowconv_launch, smfft_amd.rowconv; one kernel per inner length M = 256 ... 4096)
against the sum of the definition in fp64 (tools/rowconv_model.py `direct`): Gaussian row pairs on both sides of every M boundary, with
n_a and with n_b above M / 2, in both modes; exact probes (impulses, the autocorrelation of one buffer, NaN and zero rows); windows,
which must be slices of the full result to the bit; the grid size, which must not show in the bits; the grid-stride loop; guarded
buffers at interior bases; 64-bit offsets on either input side and on the output side; a caller's stream, the benchmark form and the
host round trip.

Every run goes into an output prefilled with 0xFF (NaN), with a guard of 4096 elements of 0x5A on both sides that must stay untouched;
inputs end where their allocation ends.

The bound for full outputs, per row against fp64: ||d||_2 / ||want||_2 <= ROW_REL_L2 and max |d| / max |want| <= ROW_MAX, the FIR
bank's bounds (tests/fir_gpu_harness.py) for the same chain of a forward transform, a product and an inverse transform.  An fp32 NumPy
model of the chain (tools/rowconv_model.py `model` with complex64) gave relL2 <= 1.4e-7 and max |d| / max |want| <= 2.2e-7 on Gaussian
rows: full Gaussian rows are well conditioned and none is drawn again.  Windowed outputs are not judged by a relative bound -- a narrow
window can lie where the row's outputs are small -- but must equal the same elements of the full launch to the bit.  The one exception
is the two m = 1 cases of the 64-bit offset test, where a full launch would need 16 GiB twice over: there the bound is the row bound on
the one output, and a row pair is drawn again while that output is below half its expectation, |want| < ||full want||_2 / (2 sqrt(Lfull)),
judged from the fp64 reference alone and never from the kernel's output (the error of the chain scales with the whole row, so it is
relative to one output only where that output is of the row's size).  The tests print the worst figures they measure per M.

The file's name makes it collect behind every older GPU test file, so that each of those keeps its place in a run of the suite."""
import ctypes
import os
import sys

import numpy as np
import pytest

from tests import rows_gpu_harness as rh
from tests.fir_gpu_harness import GRID_CAP, GUARD, ROW_MAX, ROW_REL_L2

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import rowconv_model as rm  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [256, 512, 1024, 2048, 4096]
LARGEST = {256: (128, 129), 512: (256, 257), 1024: (512, 513), 2048: (1024, 1025), 4096: (2048, 2049)}      # n_a + n_b - 1 = M
MODES = (False, True)       # correlate
WORST = rh.Worst()      # M -> [relL2, max / max]: the worst figures measured in this run


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def rc():
    from smfft_amd import rowconv
    rowconv.lib()
    return rowconv


def _mode(correlate):
    return "correlate" if correlate else "convolve"


def _check_rows(got, want, M, what):
    """got, want: (batch, m); prints the worst row figures before it asserts"""
    d = got.astype(np.complex128) - want
    l2 = np.linalg.norm(d, axis=1) / np.maximum(np.linalg.norm(want, axis=1), 1e-30)
    mx = np.max(np.abs(d), axis=1) / np.maximum(np.max(np.abs(want), axis=1), 1e-30)
    worst = WORST.record(M, l2, mx)
    print(f"{what}: worst row relL2 = {l2.max():.3e}, max |d| / max |want| = {mx.max():.3e}  (M = {M} so far: {worst[0]:.3e}, {worst[1]:.3e})")
    assert l2.max() <= ROW_REL_L2 and mx.max() <= ROW_MAX, f"{what}: row {int(np.argmax(l2))} relL2 = {l2.max():.3e}, row {int(np.argmax(mx))} max = {mx.max():.3e}"


def run(sm, rc, a, b, correlate, first=0, m=None, front=0, finite=True, launch=None):
    """one launch through the device-pointer API on copies of a = (batch, n_a) and b = (batch, n_b) complex64 that end where their
    allocations end; b = None: d_b = d_a, one buffer for both.  Returns the (batch, m) result after checking the guards and (finite)
    that no NaN of the prefill is left.  m = None: the full result behind `first`.  front: elements between the output's front guard
    and the output's base; launch(da, db, dout, n_a, n_b, first, m, batch, correlate): how to launch, when not on the null stream
    through the mirror"""
    a = np.ascontiguousarray(a)
    assert a.dtype == np.complex64 and a.ndim == 2
    batch, n_a = a.shape
    da = sm.DeviceBuffer.from_host(a)
    assert da.nbytes == a.nbytes
    if b is None:
        db, pb, n_b = None, da.ptr, n_a
    else:
        b = np.ascontiguousarray(b)
        assert b.dtype == np.complex64 and b.shape[0] == batch
        n_b = b.shape[1]
        db = sm.DeviceBuffer.from_host(b)
        assert db.nbytes == b.nbytes
        pb = db.ptr
    first, m = rm.window(n_a, n_b, first, m)
    dout, pout = rh.guarded(sm, batch * m, 8, front)
    try:
        if launch is None:
            rc.launch(da.ptr, pb, pout, n_a, n_b, first, m, batch, correlate)
        else:
            launch(da.ptr, pb, pout, n_a, n_b, first, m, batch, correlate)
        assert sm.lib.smfft_synchronize() == 0
        return rh.collect(dout, batch * m, np.complex64, front, finite).reshape(batch, m)
    finally:
        for buf in (da, db, dout):
            if buf is not None:
                buf.free()


def _ffts(n_a, n_b):
    return 4096 // rm.fft_size(n_a, n_b)


def _batch(n_a, n_b, tiles=2, extra=1):
    return tiles * _ffts(n_a, n_b) + extra


# ---- 1: fp64 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_a, n_b", [(1, 1), (1, 256), (256, 1), (128, 129), (129, 129),            # M boundaries, degenerate rows
                                      (300, 200), (200, 300),                                          # n_a > M / 2, n_b > M / 2
                                      (1000, 25), (1000, 26),                                          # the 1024 / 2048 boundary
                                      (4095, 2), (2, 4095),                                            # a thread's last element, on either side
                                      (4096, 1), (1, 4096), (2048, 2049),                              # the largest, the degenerate large
                                      (1536, 513)])                                                    # asymmetric and large
def test_against_fp64(sm, rc, n_a, n_b):
    """batch = 2F + 1 (two full tiles and one row), the full output, both modes"""
    rng = np.random.default_rng(1000 * n_a + n_b)
    batch = _batch(n_a, n_b)
    a, b = rh.rand(rng, (batch, n_a), np.complex64), rh.rand(rng, (batch, n_b), np.complex64)
    for correlate in MODES:
        got = run(sm, rc, a, b, correlate)
        assert got.shape == (batch, n_a + n_b - 1)
        _check_rows(got, rm.direct(a, b, correlate), rm.fft_size(n_a, n_b), f"n_a={n_a} n_b={n_b} {_mode(correlate)}")


# ---- 2: exact probes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_a, n_b", [(300, 200), (128, 129), (1000, 25), (2048, 2049), (1536, 513)])
def test_probe_impulses(sm, rc, n_a, n_b):
    """row r of a = a unit impulse at j0 in {0, 1, n_a / 2, n_a - 1}, b Gaussian: the output is b (convolve) or its reversed conjugate
    (correlate) at j0 ... j0 + n_b - 1 and zero elsewhere, every element within ROW_MAX max |b|.  (The last shape puts an impulse
    through the kernel of M = 2048 too.)"""
    js = sorted({0, 1, n_a // 2, n_a - 1})
    rng = np.random.default_rng(40 + n_a)
    a = np.zeros((len(js), n_a), np.complex64)
    a[np.arange(len(js)), js] = 1
    b = rh.rand(rng, (len(js), n_b), np.complex64)
    for correlate in MODES:
        got = run(sm, rc, a, b, correlate).astype(np.complex128)
        second = rm.second_operand(b.astype(np.complex128), correlate)
        for r, j0 in enumerate(js):
            want = np.zeros(n_a + n_b - 1, np.complex128)
            want[j0:j0 + n_b] = second[r]
            err, scale = np.max(np.abs(got[r] - want)), np.max(np.abs(b[r]))
            print(f"n_a={n_a} n_b={n_b} {_mode(correlate)} impulse at {j0}: max |d| / max |b| = {err / scale:.3e}")
            assert err <= ROW_MAX * scale, (n_a, n_b, correlate, j0, err / scale)


@pytest.mark.parametrize("n", [129, 2048])
def test_probe_autocorrelation(sm, rc, n):
    """d_a == d_b with correlate set, batch = 2F + 1: the fp64 autocorrelation within the row bounds; lag 0, at index n - 1, is ||a||^2
    within ROW_MAX ||a||^2; and the bits are those of two buffers with the same content"""
    rng = np.random.default_rng(45 + n)
    a = rh.rand(rng, (_batch(n, n), n), np.complex64)
    got = run(sm, rc, a, None, True)
    assert got.shape == (a.shape[0], 2 * n - 1)
    _check_rows(got, rm.direct(a, a, True), rm.fft_size(n, n), f"autocorrelation n={n}")
    energy = np.sum(np.abs(a.astype(np.complex128)) ** 2, axis=1)
    err = np.abs(got[:, n - 1].astype(np.complex128) - energy) / energy
    print(f"autocorrelation n={n}: worst |y[n - 1] - ||a||^2| / ||a||^2 = {err.max():.3e}")
    assert err.max() <= ROW_MAX, (n, err.max())
    assert np.array_equal(rh.bits(got), rh.bits(run(sm, rc, a, a.copy(), True))), n


# ---- 3: the window ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_a, n_b", [(300, 200), (2048, 2049), (1, 4096)])
def test_window(sm, rc, n_a, n_b):
    """(first, m) in {(0, 1), (Lfull - 1, 1), (n_b - 1 - 3, 7) where it fits (the lags -3 ... 3), (1, Lfull - 2)}, batch = 2F + 1, both
    modes: the bits of the slice of the full run, which passes the fp64 bound; the guards on both sides of the batch * m outputs stay"""
    full = n_a + n_b - 1
    windows = [(0, 1), (full - 1, 1), (1, full - 2)] + ([(n_b - 4, 7)] if n_b - 4 >= 0 and n_b + 3 <= full else [])
    assert (len(windows) == 3) == ((n_a, n_b) == (1, 4096))
    rng = np.random.default_rng(55 + n_a)
    batch = _batch(n_a, n_b)
    a, b = rh.rand(rng, (batch, n_a), np.complex64), rh.rand(rng, (batch, n_b), np.complex64)
    for correlate in MODES:
        base = run(sm, rc, a, b, correlate)
        _check_rows(base, rm.direct(a, b, correlate), rm.fft_size(n_a, n_b), f"n_a={n_a} n_b={n_b} {_mode(correlate)} full")
        for first, m in windows:
            got = run(sm, rc, a, b, correlate, first=first, m=m)
            assert got.shape == (batch, m)
            assert np.array_equal(rh.bits(got), rh.bits(base[:, first:first + m])), (n_a, n_b, correlate, first, m)


# ---- 4: isolation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_a, n_b", [(128, 129), (300, 200), (2048, 2049)])
def test_probe_rows_are_isolated(sm, rc, n_a, n_b):
    """batch = 3F, three runs per mode: one row of a all NaN; one row of b with a single NaN sample; one row of a all zero.  The
    poisoned row is NaN in all its outputs, the zero row's are +0 bits, and every other row keeps the bits of the clean run"""
    F = _ffts(n_a, n_b)
    rng = np.random.default_rng(50 + n_a)
    a, b = rh.rand(rng, (3 * F, n_a), np.complex64), rh.rand(rng, (3 * F, n_b), np.complex64)
    whole, single, zero = F + F // 2, 2 * F + F // 3, F // 5
    assert len({whole, single, zero}) == 3
    for correlate in MODES:
        clean = run(sm, rc, a, b, correlate)
        _check_rows(clean, rm.direct(a, b, correlate), rm.fft_size(n_a, n_b), f"n_a={n_a} n_b={n_b} {_mode(correlate)} clean")
        for case, row in (("a all NaN", whole), ("b one NaN", single), ("a all zero", zero)):
            bad_a, bad_b = a.copy(), b.copy()
            if case == "a all NaN":
                bad_a[row] = np.nan
            elif case == "b one NaN":
                bad_b[row, n_b // 3] = np.complex64(complex(np.nan, bad_b[row, n_b // 3].imag))
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


# ---- 5: the grid --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", SIZES)
def test_grid_is_invisible(sm, rc, M):
    """the largest shape of M (Lfull = M), batch = 5F + 1 (six tiles), both modes: launch_tuned on 1, 2, 3, 6 and 12288 workgroups gives
    the bits of launch.  One workgroup runs all six tiles"""
    n_a, n_b = LARGEST[M]
    assert rm.fft_size(n_a, n_b) == M and n_a + n_b - 1 == M
    rng = np.random.default_rng(60 + M)
    batch = _batch(n_a, n_b, 5)
    a, b = rh.rand(rng, (batch, n_a), np.complex64), rh.rand(rng, (batch, n_b), np.complex64)
    for correlate in MODES:
        base = run(sm, rc, a, b, correlate)
        _check_rows(base, rm.direct(a, b, correlate), M, f"M={M} n_a={n_a} n_b={n_b} {_mode(correlate)} six tiles")
        for grid in (1, 2, 3, 6, 12288):
            got = run(sm, rc, a, b, correlate, launch=lambda da, db, dout, na, nb, first, m, bt, c: rc.launch_tuned(da, db, dout, na, nb, first, m, bt, grid, c))
            assert np.array_equal(rh.bits(got), rh.bits(base)), (M, correlate, grid)


@pytest.mark.parametrize("n_a, n_b, batch, correlate", [(5, 3, 16 * (2 * 12288) + 7, False), (1025, 1024, 2 * 12288 + 1, True)])
def test_grid_stride_loop(sm, rc, n_a, n_b, batch, correlate):
    """more tiles than the grid cap through the plain launch: at (5, 3), M = 256, every workgroup runs two or three tiles of sixteen
    rows; at (1025, 1024), M = 2048, one workgroup runs a second tile, the partial last one.  Every row against fp64: at (5, 3) the
    sum itself; at (1025, 1024), where the sum over 24577 rows would take a minute, the fp64 chain (rm.model in complex128, which
    tests/test_sm_rowconv_cpu.py holds within 1e-12 of `direct`) and the rows of the first, the wrapping and the last tiles against
    the sum"""
    F = _ffts(n_a, n_b)
    assert GRID_CAP == 12288 and GRID_CAP < -(-batch // F) <= 3 * GRID_CAP and batch % F
    rng = np.random.default_rng(12288 + n_a)
    a, b = rh.rand(rng, (batch, n_a), np.complex64), rh.rand(rng, (batch, n_b), np.complex64)
    got = run(sm, rc, a, b, correlate)
    M = rm.fft_size(n_a, n_b)
    what = f"grid-stride n_a={n_a} n_b={n_b} batch={batch} {_mode(correlate)}"
    if min(n_a, n_b) <= 16:
        _check_rows(got, rm.direct(a, b, correlate), M, what)
    else:
        _check_rows(got, rm.model(a, b, correlate), M, what + ", fp64 chain")
        rows = sorted({0, F - 1, GRID_CAP * F - 1, GRID_CAP * F, 2 * GRID_CAP * F - 1, 2 * GRID_CAP * F, batch - 1} & set(range(batch)))
        _check_rows(got[rows], rm.direct(a[rows], b[rows], correlate), M, what + f", rows {rows}, the sum")


# ---- 6: bounds and placement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_a, n_b, correlate", [(300, 200, True), (1, 4096, False), (4096, 1, True)])
def test_bounds(sm, rc, n_a, n_b, correlate):
    """batch in {1, F - 1, F + 1}, the inputs ending where their allocations end, the output base 1 and 3 elements behind its front
    guard: nothing in front of or behind the output changes, every output is written, and the bits are those at the aligned base,
    which pass the fp64 bound"""
    F = _ffts(n_a, n_b)
    rng = np.random.default_rng(70 + n_a)
    for batch in sorted({1, F + 1} | ({F - 1} if F > 1 else set())):
        a, b = rh.rand(rng, (batch, n_a), np.complex64), rh.rand(rng, (batch, n_b), np.complex64)
        base = run(sm, rc, a, b, correlate)
        _check_rows(base, rm.direct(a, b, correlate), rm.fft_size(n_a, n_b), f"n_a={n_a} n_b={n_b} batch={batch}")
        for front in (1, 3):
            got = run(sm, rc, a, b, correlate, front=front)
            assert np.array_equal(rh.bits(got), rh.bits(base)), f"n_a={n_a} n_b={n_b} batch={batch} front={front}: the result depends on placement"
            window = run(sm, rc, a, b, correlate, first=n_b - 1, m=1, front=front)            # lag 0 alone, at an odd base
            assert np.array_equal(rh.bits(window), rh.bits(base[:, n_b - 1:n_b])), (n_a, n_b, batch, front)


# ---- 7: 64-bit offsets ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_a, n_b, first, m, correlate", [(4095, 2, 2047, 1, False), (2, 4095, 2047, 1, True), (2048, 2048, 0, 4095, True)])
def test_offsets_beyond_two_to_the_31(sm, rc, n_a, n_b, first, m, correlate):
    """batch = ceil(2^31 / 4095) + 8 rows: 16 GiB of a (n_a = 4095), of b (n_b = 4095, read backwards under the conjugate) or of
    output (m = 4095).  The inputs are memset to zero, with Gaussian rows at row 0, at the row that straddles element 2^31 of the large
    side and at the last two rows: those rows pass the bound (the m = 1 rows drawn well conditioned, see the head of the file), zero
    rows give exactly +0 (all of them where m = 1, sampled ones where the output is the large side), every one of them was written
    over the 0xFF prefill, and the guard behind the output is intact"""
    big = max(n_a, n_b, m)
    assert big == 4095
    batch = -(-(1 << 31) // big) + 8
    straddle = (1 << 31) // big
    assert straddle * big < (1 << 31) < (straddle + 1) * big and (batch - 2) * big > (1 << 31)
    rows = [0, straddle, batch - 2, batch - 1]
    zeros = [1, straddle // 2, straddle - 1, straddle + 1, batch - 3]
    full = n_a + n_b - 1
    rng = np.random.default_rng(31 + n_a)
    a, b = rh.rand(rng, (len(rows), n_a), np.complex64), rh.rand(rng, (len(rows), n_b), np.complex64)
    want_full = rm.direct(a, b, correlate)
    while m < full:       # (m = 1: a pair whose one output is below half its expectation is drawn again)
        small = np.linalg.norm(want_full[:, first:first + m], axis=1) < 0.5 * np.sqrt(m / full) * np.linalg.norm(want_full, axis=1)
        if not small.any():
            break
        a[small], b[small] = rh.rand(rng, (int(small.sum()), n_a), np.complex64), rh.rand(rng, (int(small.sum()), n_b), np.complex64)
        want_full = rm.direct(a, b, correlate)
    want = want_full[:, first:first + m]
    da, db = sm.DeviceBuffer(batch * n_a * 8), sm.DeviceBuffer(batch * n_b * 8)
    dout = sm.DeviceBuffer((batch * m + GUARD) * 8)
    try:
        assert sm.lib.smfft_memset(da.ptr, 0, batch * n_a * 8) == 0
        assert sm.lib.smfft_memset(db.ptr, 0, batch * n_b * 8) == 0
        assert sm.lib.smfft_memset(dout.ptr, 0xFF, batch * m * 8) == 0
        assert sm.lib.smfft_memset(dout.ptr + batch * m * 8, 0x5A, GUARD * 8) == 0
        for i, r in enumerate(rows):
            assert sm.lib.smfft_memcpy_h2d(da.ptr + r * n_a * 8, a[i].ctypes.data, n_a * 8) == 0
            assert sm.lib.smfft_memcpy_h2d(db.ptr + r * n_b * 8, b[i].ctypes.data, n_b * 8) == 0
        rc.launch(da.ptr, db.ptr, dout.ptr, n_a, n_b, first, m, batch, correlate)
        assert sm.lib.smfft_synchronize() == 0
        guard = np.empty(2 * GUARD, np.uint32)
        assert sm.lib.smfft_memcpy_d2h(guard.ctypes.data, dout.ptr + batch * m * 8, guard.nbytes) == 0
        assert np.all(guard == 0x5A5A5A5A), "the kernel wrote past its output"
        got = np.empty((len(rows), m), np.complex64)
        for i, r in enumerate(rows):
            assert sm.lib.smfft_memcpy_d2h(got[i].ctypes.data, dout.ptr + r * m * 8, m * 8) == 0
        _check_rows(got, want, 4096, f"2^31 rows n_a={n_a} n_b={n_b} first={first} m={m} {_mode(correlate)}")
        if m == 1:
            whole = np.empty(batch, np.complex64)
            assert sm.lib.smfft_memcpy_d2h(whole.ctypes.data, dout.ptr, whole.nbytes) == 0
            words = rh.bits(np.delete(whole, rows))
            print(f"{words.size // 2} zero rows: {int(np.count_nonzero(words))} words that are not +0")
            assert not words.any(), "a zero row is not +0"
        else:
            for r in zeros:
                row = np.empty(m, np.complex64)
                assert sm.lib.smfft_memcpy_d2h(row.ctypes.data, dout.ptr + r * m * 8, m * 8) == 0
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
        a, b = rh.rand(rng, (37, n_a), np.complex64), rh.rand(rng, (37, n_b), np.complex64)

        def launch(da, db, dout, na, nb, first, m, batch, c):
            assert sm.lib.smfft_synchronize() == 0                              # the prefill of the output, on the null stream
            rc.launch(da, db, dout, na, nb, first, m, batch, c, stream=stream.value)
            assert hip.hipStreamSynchronize(stream) == 0
        _check_rows(run(sm, rc, a, b, correlate, launch=launch), rm.direct(a, b, correlate), rm.fft_size(n_a, n_b), f"stream n_a={n_a} n_b={n_b}")
    assert hip.hipStreamDestroy(stream) == 0


def test_benchmark_form_adds_to_the_timer(sm, rc):
    """the library's smfft_rowconv_benchmark adds its milliseconds to a non-zero total and fills the output; so does the mirror's"""
    n_a, n_b = 1536, 513
    rng = np.random.default_rng(12)
    a, b = rh.rand(rng, (300, n_a), np.complex64), rh.rand(rng, (300, n_b), np.complex64)
    total = ctypes.c_double(1.0)

    def c_form(da, db, dout, na, nb, first, m, batch, c):
        assert rc.lib().smfft_rowconv_benchmark(da, db, dout, na, nb, first, m, batch, int(c), ctypes.byref(total)) == 0
        assert total.value > 1.0
    out = run(sm, rc, a, b, True, launch=c_form)
    _check_rows(out, rm.direct(a, b, True), 2048, "benchmark form")

    def mirror(da, db, dout, na, nb, first, m, batch, c):
        status, ms = rc.benchmark(da, db, dout, na, nb, first, m, batch, c)
        assert status == 0 and ms > 0.0
    assert np.array_equal(rh.bits(run(sm, rc, a, b, True, launch=mirror)), rh.bits(out))


def test_host_round_trip(sm, rc):
    """rowconv.convolve on 1-D, 3-D, float64 and real inputs against np.convolve and np.correlate: complex64 of shape (..., m), the bits
    of the device-pointer launch; a window is its slice; an empty batch returns an empty array"""
    rng = np.random.default_rng(7)
    a1 = rng.standard_normal(1000) + 1j * rng.standard_normal(1000)                  # 1-D complex128
    b1 = rng.standard_normal(25) + 1j * rng.standard_normal(25)
    a32, b32 = a1.astype(np.complex64), b1.astype(np.complex64)
    got = rc.convolve(a1, b1)
    assert got.shape == (1024,) and got.dtype == np.complex64
    assert np.array_equal(rh.bits(got), rh.bits(run(sm, rc, a32[None], b32[None], False)[0]))
    _check_rows(got[None], np.convolve(a32.astype(np.complex128), b32.astype(np.complex128))[None], 1024, "convolve() 1-D against np.convolve")
    got = rc.convolve(a1, b1, correlate=True)
    _check_rows(got[None], np.correlate(a32.astype(np.complex128), b32.astype(np.complex128), "full")[None], 1024, "convolve() 1-D against np.correlate")
    lags = rc.convolve(a1, b1, correlate=True, first=25 - 1 - 16, m=33)              # the lags -16 ... 16
    assert lags.shape == (33,) and np.array_equal(rh.bits(lags), rh.bits(got[8:41]))
    tail = rc.convolve(a1, b1, first=1000)
    assert tail.shape == (24,) and np.array_equal(rh.bits(tail), rh.bits(rc.convolve(a1, b1)[1000:]))
    a3, b3 = rh.rand(rng, (2, 3, 257), np.complex64), rh.rand(rng, (2, 3, 100), np.complex64)
    got = rc.convolve(a3, b3, correlate=True)
    assert got.shape == (2, 3, 356) and got.dtype == np.complex64
    assert np.array_equal(rh.bits(got.reshape(6, 356)), rh.bits(run(sm, rc, a3.reshape(6, 257), b3.reshape(6, 100), True)))
    ar, br = rng.standard_normal((4, 129)), rng.standard_normal((4, 130))            # real float64
    got = rc.convolve(ar, br)
    want = np.stack([np.convolve(ar[r].astype(np.float32).astype(np.float64), br[r].astype(np.float32).astype(np.float64)) for r in range(4)])
    _check_rows(got, want.astype(np.complex128), 512, "convolve() real")
    assert got.dtype == np.complex64 and got.shape == (4, 258)
    assert np.array_equal(rh.bits(rc.convolve(ar.astype(np.float32), br.astype(np.float32))), rh.bits(got))
    empty = rc.convolve(np.zeros((0, 5), np.complex64), np.zeros((0, 3), np.complex64))
    assert empty.shape == (0, 7) and empty.dtype == np.complex64
    assert ROW_REL_L2 == 1e-6 and ROW_MAX == 5e-6

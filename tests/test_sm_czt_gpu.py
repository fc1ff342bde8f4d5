"""The chirp-z transforms on an MI355X (smfft_czt_launch, smfft_amd.czt; one kernel per inner length M = 256 ... 4096) against the
O(n m) sum of the definition in fp64 (tools/czt_model.py `direct`): Gaussian rows on both sides of every M boundary, with n and with m
above M / 2, on four arcs; exact probes (impulses, tones, NaN rows); the grid size, which must not show in the bits; the grid-stride
loop; guarded buffers at interior bases; in-place calls at m = n; 64-bit offsets on the input and on the output side; a caller's
stream, the benchmark form and the host round trip.

Every run goes into an output prefilled with 0xFF (NaN), with a guard of 4096 elements of 0x5A on both sides that must stay untouched;
inputs end where their allocation ends.

The bound, per row against fp64: ||d||_2 / ||want||_2 <= ROW_REL_L2 and max |d| / max |want| <= ROW_MAX, the FIR bank's and the
Bluestein library's bounds (tests/fir_gpu_harness.py) for the same chain of a forward transform, a product with a prepared spectrum and
an inverse transform.  An fp32 NumPy model of the chain gave relL2 <= 1.6e-7 and max |d| / max |want| <= 4.7e-7 over Gaussian rows at
the shapes of tests/test_sm_czt_cpu.py, so the bounds leave the margin the Bluestein tests leave.  The tests print the worst figures
they measure per M.

The rows are Gaussian and well conditioned (`_rows`): the bound is relative to a row's own outputs, and with few outputs, or with many
that lie within one resolution cell of each other, a Gaussian row can cancel in all of them at once -- at m = 1 the one output is
below a fifth of ||x||_2 in one row of twenty-five, and there the fp32 model itself is at relL2 = 3.4e-6 (row 20 of the first draw at
(256, 1): |X| = 0.61, ||x||_2 = 22.2) although its absolute error is the usual 1e-7 ||x||_2.  That is the cancellation the tone test
judges against n.  So a row whose outputs on one of the test's arcs fall below half their expectation,
||want||_2 < sqrt(m) ||x||_2 / 2, is drawn again; this looks at the input and the fp64 reference alone, never at the kernel's output.

The file's name makes it collect behind every older GPU test file, so that each of those keeps its place in a run of the suite."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

from tests import rows_gpu_harness as rh
from tests.fir_gpu_harness import GRID_CAP, GUARD, ROW_MAX, ROW_REL_L2

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import czt_model as cm  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [256, 512, 1024, 2048, 4096]
LARGEST = {256: (128, 129), 512: (256, 257), 1024: (512, 513), 2048: (1024, 1025), 4096: (2048, 2048)}      # n + m - 1 = M (4095 at 4096)
WORST = rh.Worst()      # M -> [relL2, max / max]: the worst figures measured in this run


def arcs(n):
    """(start, step): the DFT's arc, a zoom of eight, a coarse backward arc off every grid, and a single frequency m times over"""
    return ((0.0, 1.0 / n), (0.1, 1.0 / (8 * n)), (-0.2, -0.013), (0.37, 0.0))


def zoom(n):
    return 0.1, 1.0 / (8 * n)


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def cz():
    from smfft_amd import czt
    czt.lib()
    return czt


@functools.lru_cache(maxsize=3)
def _kernel(n, m, start, step):
    """(n, m) complex128: exp(-2 pi i j (start + k step)), computed once per arc and shared, read only"""
    w = cm.unit(-cm.phases(n, m, start, step))
    w.setflags(write=False)
    return w


def _want(x, m, start, step):
    """cm.direct with the matrix of the arc shared among the tests"""
    return x.astype(np.complex128) @ _kernel(x.shape[-1], m, float(start), float(step))


def _rows(rng, batch, n, m, arc_list):
    """(x, wants): x (batch, n) complex64 Gaussian rows, each drawn again until ||want||_2 >= sqrt(m) ||x||_2 / 2 on every arc of
    arc_list (E ||want||_2^2 = m ||x||_2^2: every entry of the arc's matrix has modulus 1), and the fp64 references (batch, m), one per
    arc, computed here once"""
    x = rh.rand(rng, (batch, n), np.complex64)
    wants = [np.empty((batch, m), np.complex128) for _ in arc_list]
    todo = np.arange(batch)
    while todo.size:
        bad = np.zeros(todo.size, bool)
        floor = 0.5 * np.sqrt(m) * np.linalg.norm(x[todo].astype(np.complex128), axis=1)
        for want, (start, step) in zip(wants, arc_list):
            want[todo] = _want(x[todo], m, start, step)
            bad |= np.linalg.norm(want[todo], axis=1) < floor
        todo = todo[bad]
        x[todo] = rh.rand(rng, (todo.size, n), np.complex64)
    return x, wants


def _check_rows(got, want, n, what, rel_l2=ROW_REL_L2):
    """got, want: (batch, m); prints the worst row figures before it asserts"""
    d = got.astype(np.complex128) - want
    l2 = np.linalg.norm(d, axis=1) / np.maximum(np.linalg.norm(want, axis=1), 1e-30)
    mx = np.max(np.abs(d), axis=1) / np.maximum(np.max(np.abs(want), axis=1), 1e-30)
    M = cm.fft_size(n, got.shape[1])
    worst = WORST.record(M, l2, mx)
    print(f"{what}: worst row relL2 = {l2.max():.3e}, max |d| / max |want| = {mx.max():.3e}  (M = {M} so far: {worst[0]:.3e}, {worst[1]:.3e})")
    assert l2.max() <= rel_l2 and mx.max() <= ROW_MAX, f"{what}: row {int(np.argmax(l2))} relL2 = {l2.max():.3e}, row {int(np.argmax(mx))} max = {mx.max():.3e}"


class Plan:
    """the prepared plan of (n, m, start, step) on the device"""

    def __init__(self, sm, cz, n, m, start, step, stream=0):
        self.buf = sm.DeviceBuffer(cz.plan_bytes(n, m))
        cz.prepare(n, m, start, step, self.buf.ptr, stream=stream)
        self.ptr = self.buf.ptr

    def free(self):
        self.buf.free()


def run(sm, cz, x, m, start, step, front=0, finite=True, launch=None, in_place=False):
    """one launch through the device-pointer API on a copy of x = (batch, n) complex64 that ends where its allocation ends; returns the
    (batch, m) result after checking the guards and (finite) that no NaN of the prefill is left.  front: elements between the output's
    front guard and the output's base; launch(din, dout, n, m, batch, plan): how to launch, when not on the null stream through the
    mirror; in_place (m == n): the input is copied into the guarded buffer, which is input and output"""
    x = np.ascontiguousarray(x)
    assert x.dtype == np.complex64 and x.ndim == 2
    batch, n = x.shape
    plan = Plan(sm, cz, n, m, start, step)
    dout, pout = rh.guarded(sm, batch * m, 8, front)
    if in_place:
        assert m == n
        din, pin = None, pout
        assert sm.lib.smfft_memcpy_h2d(pout, x.ctypes.data, x.nbytes) == 0
    else:
        din = sm.DeviceBuffer.from_host(x)
        assert din.nbytes == x.nbytes
        pin = din.ptr
    try:
        if launch is None:
            cz.launch(pin, pout, n, m, batch, plan.ptr)
        else:
            launch(pin, pout, n, m, batch, plan.ptr)
        assert sm.lib.smfft_synchronize() == 0
        return rh.collect(dout, batch * m, np.complex64, front, finite).reshape(batch, m)
    finally:
        for b in (din, dout, plan):
            if b is not None:
                b.free()


def _ffts(n, m):
    return 4096 // cm.fft_size(n, m)


def _batch(n, m, tiles=2, extra=1):
    return tiles * _ffts(n, m) + extra


# ---- 1: fp64 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, m", [(1, 1), (1, 256), (256, 1), (257, 1), (128, 129), (128, 130),        # M boundaries, degenerate rows
                                  (300, 200), (200, 300),                                               # n > M / 2, m > M / 2
                                  (1000, 24), (1000, 25), (1000, 26),                                   # the 1024 / 2048 boundary
                                  (2047, 2), (2, 2047),                                                 # a thread's last element, in and out
                                  (2048, 1), (1, 2048), (2048, 2048),                                   # the largest, the degenerate large
                                  (1536, 513)])                                                         # asymmetric and large
def test_against_fp64(sm, cz, n, m):
    """batch = 2F + 1 (two full tiles and one row) on the four arcs; on the DFT's arc with m = n also against np.fft, both directions"""
    rng = np.random.default_rng(1000 * n + m)
    x, wants = _rows(rng, _batch(n, m), n, m, arcs(n))
    for (start, step), want in zip(arcs(n), wants):
        got = run(sm, cz, x, m, start, step)
        _check_rows(got, want, n, f"n={n} m={m} start={start} step={step:.3g}")
    if m == n:
        x64 = x.astype(np.complex128)
        _check_rows(run(sm, cz, x, n, 0.0, 1.0 / n), np.fft.fft(x64, axis=-1), n, f"n={n} against np.fft.fft")
        _check_rows(run(sm, cz, x, n, 0.0, -1.0 / n), np.fft.ifft(x64, axis=-1) * n, n, f"n={n} against np.fft.ifft n")


# ---- 2 - 4: exact probes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, m", [(300, 200), (2048, 2048), (128, 129), (1000, 25), (1536, 513)])
def test_probe_impulses(sm, cz, n, m):
    """row r = an impulse at j in {0, 1, n / 2, n - 1}: X[k] = exp(-2 pi i j (start + k step)), every element within ROW_MAX of its value
    of modulus 1, on the four arcs.  This reaches every entry of A and C and both ends of b's support.  (The last three shapes put an
    impulse through the kernels of M = 256, 1024 and 2048 too.)"""
    js = sorted({0, 1, n // 2, n - 1})
    x = np.zeros((len(js), n), np.complex64)
    x[np.arange(len(js)), js] = 1
    for start, step in arcs(n):
        got = run(sm, cz, x, m, start, step).astype(np.complex128)
        want = _kernel(n, m, float(start), float(step))
        for r, j in enumerate(js):
            err = np.max(np.abs(got[r] - want[j]))
            print(f"n={n} m={m} start={start} step={step:.3g} impulse at {j}: max |d| = {err:.3e}")
            assert err <= ROW_MAX, (n, m, start, step, j, err)


def test_probe_tones(sm, cz):
    """n = 2048, m = 256, start = 0.1, step = 1 / 16384, x a unit tone at f: on the first bin (a peak of n at k = 0), between two bins
    (f = start + 100.5 step) and out of band (f = 0.3).  Every |d| <= ROW_MAX n: the out-of-band outputs are about 1e-3 n by
    cancellation, so they are judged against n, not against ||want|| (an fp32 model of the chain is at relL2 = 1.1e-6 of them, which is
    no defect).  The fp32 model gave 6e-8 n, 8e-8 n and 1.5e-9 n.  Chirp phase errors, which random input hides, show here."""
    n, m, start, step = 2048, 256, 0.1, 1.0 / 16384
    fs = (start, start + 100.5 * step, 0.3)
    j = np.arange(n, dtype=np.float64)
    x = np.stack([cm.unit(cm.cycles(f, j)) for f in fs]).astype(np.complex64)
    got = run(sm, cz, x, m, start, step).astype(np.complex128)
    want = _want(x, m, start, step)
    assert abs(want[0, 0] - n) <= 1e-4 * n and int(np.argmax(np.abs(want[0]))) == 0
    assert int(np.argmax(np.abs(want[1]))) in (100, 101) and np.max(np.abs(want[2])) <= 1e-2 * n
    for r, f in enumerate(fs):
        err = np.max(np.abs(got[r] - want[r]))
        print(f"tone at f={f:.6f}: max |d| / n = {err / n:.3e}, max |want| / n = {np.max(np.abs(want[r])) / n:.3e}")
        assert err <= ROW_MAX * n, (f, err / n)
    assert abs(got[0, 0] - n) <= ROW_MAX * n + abs(want[0, 0] - n)


@pytest.mark.parametrize("n, m", [(128, 129), (2048, 2048)])
def test_probe_rows_are_isolated(sm, cz, n, m):
    """batch = 3F: one row all NaN, and in a second run one row with a single NaN sample: the poisoned row is NaN in all m outputs and
    every other row keeps the bits of the run without NaN"""
    F = _ffts(n, m)
    start, step = zoom(n)
    rng = np.random.default_rng(50 + n)
    x, (want,) = _rows(rng, 3 * F, n, m, [(start, step)])
    clean = run(sm, cz, x, m, start, step)
    _check_rows(clean, want, n, f"n={n} m={m} clean")
    whole, single = F + F // 2, 2 * F + F // 3
    assert whole != single
    for row, sample in ((whole, None), (single, n // 3)):
        bad = x.copy()
        if sample is None:
            bad[row] = np.nan
        else:
            bad[row, sample] = np.complex64(complex(np.nan, bad[row, sample].imag))
        got = run(sm, cz, bad, m, start, step, finite=False)
        assert got.shape == (3 * F, m) and np.isnan(got[row]).all(), (n, m, row, sample, int(np.isnan(got[row]).sum()))
        others = np.arange(3 * F) != row
        assert np.array_equal(rh.bits(got[others]), rh.bits(clean[others])), (n, m, row, sample)


# ---- 5, 6: the grid -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", SIZES)
def test_grid_is_invisible(sm, cz, M):
    """the largest shape of M, batch = 5F + 1 (six tiles): launch_tuned on 1, 2, 3, 6 and 12288 workgroups gives the bits of launch.  One
    workgroup runs all six tiles with its tables held in registers (and, at M >= 2048, C in LDS)"""
    n, m = LARGEST[M]
    assert cm.fft_size(n, m) == M and (M == 4096 or n + m - 1 == M)
    start, step = zoom(n)
    rng = np.random.default_rng(60 + M)
    x, (want,) = _rows(rng, _batch(n, m, 5), n, m, [(start, step)])
    base = run(sm, cz, x, m, start, step)
    _check_rows(base, want, n, f"M={M} n={n} m={m} six tiles")
    for grid in (1, 2, 3, 6, 12288):
        got = run(sm, cz, x, m, start, step, launch=lambda din, dout, n_, m_, batch, plan: cz.launch_tuned(din, dout, n_, m_, batch, plan, grid))
        assert np.array_equal(rh.bits(got), rh.bits(base)), (M, grid)


@pytest.mark.parametrize("n, m, batch", [(5, 3, 16 * (2 * 12288) + 7), (1025, 1024, 2 * 12288 + 1)])
def test_grid_stride_loop(sm, cz, n, m, batch):
    """more tiles than the grid cap through the plain launch: at (5, 3), M = 256, every workgroup runs two or three tiles of sixteen
    rows; at (1025, 1024), M = 2048, one workgroup runs a second tile, the partial last one, with A and B in registers and C in LDS"""
    F = _ffts(n, m)
    assert GRID_CAP == 12288 and GRID_CAP < -(-batch // F) <= 3 * GRID_CAP and batch % F
    start, step = zoom(n)
    rng = np.random.default_rng(12288 + n)
    x, (want,) = _rows(rng, batch, n, m, [(start, step)])
    _check_rows(run(sm, cz, x, m, start, step), want, n, f"grid-stride n={n} m={m} batch={batch}")


# ---- 7: bounds and in-place calls ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, m", [(300, 200), (1, 2048), (2048, 1)])
def test_bounds(sm, cz, n, m):
    """batch in {1, F - 1, F + 1}, the input ending where its allocation ends, the output base 1 and 3 elements behind its front guard:
    nothing in front of or behind the output changes, every output is written, and the bits are those at the aligned base, which pass
    the fp64 bound"""
    F = _ffts(n, m)
    start, step = zoom(n)
    rng = np.random.default_rng(70 + n)
    for batch in sorted({1, F + 1} | ({F - 1} if F > 1 else set())):
        x, (want,) = _rows(rng, batch, n, m, [(start, step)])
        base = run(sm, cz, x, m, start, step)
        _check_rows(base, want, n, f"n={n} m={m} batch={batch}")
        for front in (1, 3):
            got = run(sm, cz, x, m, start, step, front=front)
            assert np.array_equal(rh.bits(got), rh.bits(base)), f"n={n} m={m} batch={batch} front={front}: the result depends on placement"


@pytest.mark.parametrize("n", [129, 2047])
def test_in_place(sm, cz, n):
    """d_out == d_in at m = n, batch = 2F + 1: the bits of the out-of-place run"""
    start, step = zoom(n)
    rng = np.random.default_rng(80 + n)
    x, (want,) = _rows(rng, _batch(n, n), n, n, [(start, step)])
    base = run(sm, cz, x, n, start, step)
    _check_rows(base, want, n, f"n=m={n} out of place")
    assert np.array_equal(rh.bits(run(sm, cz, x, n, start, step, in_place=True)), rh.bits(base)), n


# ---- 8: 64-bit offsets ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, m", [(2047, 1), (1, 2047)])
def test_offsets_beyond_two_to_the_31(sm, cz, n, m):
    """batch = ceil(2^31 / 2047) + 8 rows: about 16 GiB of input (n = 2047, one output per row) or of output (m = 2047, one sample per
    row).  The input is memset to zero, with Gaussian rows at row 0, at the row that straddles element 2^31 of the large side and at
    the last two rows: those rows pass the bound, zero rows give exactly +0 (all of them where the output is the small side, sampled
    ones where it is the large one), every one of them was written over the 0xFF prefill, and the guard behind the output is intact"""
    big = max(n, m)
    batch = -(-(1 << 31) // big) + 8
    straddle = (1 << 31) // big
    assert straddle * big < (1 << 31) < (straddle + 1) * big and (batch - 2) * big > (1 << 31)
    rows = [0, straddle, batch - 2, batch - 1]
    zeros = [1, straddle // 2, straddle - 1, straddle + 1, batch - 3]
    start, step = zoom(big)
    rng = np.random.default_rng(31 + n)
    x, (want,) = _rows(rng, len(rows), n, m, [(start, step)])
    din = sm.DeviceBuffer(batch * n * 8)
    dout = sm.DeviceBuffer((batch * m + GUARD) * 8)
    plan = Plan(sm, cz, n, m, start, step)
    try:
        assert sm.lib.smfft_memset(din.ptr, 0, batch * n * 8) == 0
        assert sm.lib.smfft_memset(dout.ptr, 0xFF, batch * m * 8) == 0
        assert sm.lib.smfft_memset(dout.ptr + batch * m * 8, 0x5A, GUARD * 8) == 0
        for i, r in enumerate(rows):
            assert sm.lib.smfft_memcpy_h2d(din.ptr + r * n * 8, x[i].ctypes.data, n * 8) == 0
        cz.launch(din.ptr, dout.ptr, n, m, batch, plan.ptr)
        assert sm.lib.smfft_synchronize() == 0
        guard = np.empty(2 * GUARD, np.uint32)
        assert sm.lib.smfft_memcpy_d2h(guard.ctypes.data, dout.ptr + batch * m * 8, guard.nbytes) == 0
        assert np.all(guard == 0x5A5A5A5A), "the kernel wrote past its output"
        got = np.empty((len(rows), m), np.complex64)
        for i, r in enumerate(rows):
            assert sm.lib.smfft_memcpy_d2h(got[i].ctypes.data, dout.ptr + r * m * 8, m * 8) == 0
        _check_rows(got, want, n, f"2^31 rows n={n} m={m}")
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
        for b in (din, dout, plan):
            b.free()


# ---- 9: entry forms ---------------------------------------------------------------------------------------------------------------------
def test_caller_stream(sm, cz):
    """prepare and launch on a stream from hipStreamCreate, then hipStreamSynchronize"""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value
    rng = np.random.default_rng(11)
    for n, m in ((1000, 24), (100, 300)):
        start, step = zoom(n)
        x, (want,) = _rows(rng, 37, n, m, [(start, step)])

        def launch(din, dout, n_, m_, batch, plan):
            mine = Plan(sm, cz, n_, m_, start, step, stream=stream.value)       # (the run's own plan goes unused)
            assert sm.lib.smfft_synchronize() == 0                              # the prefill of the output, on the null stream
            cz.launch(din, dout, n_, m_, batch, mine.ptr, stream=stream.value)
            assert hip.hipStreamSynchronize(stream) == 0
            mine.free()
        _check_rows(run(sm, cz, x, m, start, step, launch=launch), want, n, f"stream n={n} m={m}")
    assert hip.hipStreamDestroy(stream) == 0


def test_benchmark_form_adds_to_the_timer(sm, cz):
    """the library's smfft_czt_benchmark adds its milliseconds to a non-zero total and fills the output; so does the mirror's"""
    n, m = 1536, 513
    start, step = zoom(n)
    rng = np.random.default_rng(12)
    x, (want,) = _rows(rng, 300, n, m, [(start, step)])
    total = ctypes.c_double(1.0)

    def c_form(din, dout, n_, m_, batch, plan):
        assert cz.lib().smfft_czt_benchmark(din, dout, n_, m_, batch, plan, ctypes.byref(total)) == 0
        assert total.value > 1.0
    out = run(sm, cz, x, m, start, step, launch=c_form)
    _check_rows(out, want, n, "benchmark form")

    def mirror(din, dout, n_, m_, batch, plan):
        rc, ms = cz.benchmark(din, dout, n_, m_, batch, plan)
        assert rc == 0 and ms > 0.0
    assert np.array_equal(rh.bits(run(sm, cz, x, m, start, step, launch=mirror)), rh.bits(out))


def test_host_round_trip(sm, cz):
    """czt.czt on 1-D, 3-D, float64 and real inputs: complex64 of shape (..., m), the bits of the device-pointer launch; the defaults
    m = n, start = 0, step = 1 / n are the DFT; an empty batch returns an empty array"""
    rng = np.random.default_rng(7)
    x1 = rng.standard_normal(1000) + 1j * rng.standard_normal(1000)                  # 1-D complex128
    got = cz.czt(x1)
    assert got.shape == (1000,) and got.dtype == np.complex64
    assert np.array_equal(rh.bits(got), rh.bits(run(sm, cz, x1.astype(np.complex64)[None], 1000, 0.0, 1.0 / 1000)[0]))
    _check_rows(got[None], np.fft.fft(x1.astype(np.complex64).astype(np.complex128))[None], 1000, "czt() 1-D, the defaults")
    got = cz.czt(x1, m=24, start=0.1, step=1e-4)
    assert got.shape == (24,) and got.dtype == np.complex64
    assert np.array_equal(rh.bits(got), rh.bits(run(sm, cz, x1.astype(np.complex64)[None], 24, 0.1, 1e-4)[0]))
    x3 = rh.rand(rng, (2, 3, 257), np.complex64)
    got = cz.czt(x3, m=100, start=-0.2, step=-0.013)
    assert got.shape == (2, 3, 100) and got.dtype == np.complex64
    assert np.array_equal(rh.bits(got.reshape(6, 100)), rh.bits(run(sm, cz, x3.reshape(6, 257), 100, -0.2, -0.013)))
    xr = rng.standard_normal((4, 129))                                               # real float64
    got = cz.czt(xr, m=130, start=0.37)
    _check_rows(got, _want(xr.astype(np.float32).astype(np.complex64), 130, 0.37, 1.0 / 129), 129, "czt() real")
    assert got.dtype == np.complex64 and got.shape == (4, 130)
    assert np.array_equal(rh.bits(cz.czt(xr.astype(np.float32), m=130, start=0.37)), rh.bits(got))
    empty = cz.czt(np.zeros((0, 5), np.complex64), m=3)
    assert empty.shape == (0, 3) and empty.dtype == np.complex64
    assert ROW_REL_L2 == 1e-6 and ROW_MAX == 5e-6

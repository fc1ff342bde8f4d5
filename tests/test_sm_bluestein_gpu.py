"""The arbitrary-length FFTs on an MI355X (smfft_bluestein_launch, smfft_amd.bluestein; one kernel per inner length M = 256 ... 4096)
against fp64 NumPy: Gaussian rows on both sides of every M boundary; exact probes (impulses, tones, NaN rows); the grid size, which
must not show in the bits; the grid-stride loop; guarded buffers at interior bases; in-place calls; 64-bit offsets; the round trip; a
caller's stream, the benchmark form and the host round trip.

Every run goes into an output prefilled with 0xFF (NaN) and followed by a guard of 4096 elements of 0x5A that must stay untouched.

The bound, per row against fp64 np.fft: ||d||_2 / ||want||_2 <= ROW_REL_L2 and max |d| / max |want| <= ROW_MAX, the FIR bank's bounds
(tests/fir_gpu_harness.py) for the same chain of a forward transform, a product with a prepared spectrum and an inverse transform.  An
fp32 NumPy model of the algorithm gave relL2 <= 1.5e-7 and max |d| / ||x||_2 <= 6.7e-7 over Gaussian rows at these lengths, and
max |d| / max |want| of about 1.2e-7 for a pure tone at n = 2048, so the bounds leave about 4 x for the engine's own rounding.  The tests
print the worst figures they measure per M.

The file's name makes it collect behind tests/test_run_fir_detect_gpu.py, so that every older GPU test keeps its place in a run of the
suite."""
import ctypes
import os
import sys

import numpy as np
import pytest

from tests import rows_gpu_harness as rh
from tests.fir_gpu_harness import GRID_CAP, GUARD, ROW_MAX, ROW_REL_L2

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import bluestein_model as bm  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [256, 512, 1024, 2048, 4096]
ENDS = [256, 4096]
LENGTHS = {256: (1, 128), 512: (129, 256), 1024: (257, 512), 2048: (513, 1024), 4096: (1025, 2048)}      # (smallest, largest) n of M
WORST = rh.Worst()      # M -> [relL2, max / max]: the worst figures measured in this run


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def bl():
    from smfft_amd import bluestein
    bluestein.lib()
    return bluestein


def _want(x, inverse):
    x = x.astype(np.complex128)
    return np.fft.ifft(x, axis=-1) * x.shape[-1] if inverse else np.fft.fft(x, axis=-1)


def _check_rows(got, want, what, rel_l2=ROW_REL_L2):
    """got, want: (batch, n); prints the worst row figures before it asserts"""
    d = got.astype(np.complex128) - want
    l2 = np.linalg.norm(d, axis=1) / np.maximum(np.linalg.norm(want, axis=1), 1e-30)
    mx = np.max(np.abs(d), axis=1) / np.maximum(np.max(np.abs(want), axis=1), 1e-30)
    m = bm.fft_size(got.shape[1])
    worst = WORST.record(m, l2, mx)
    print(f"{what}: worst row relL2 = {l2.max():.3e}, max |d| / max |want| = {mx.max():.3e}  (M = {m} so far: {worst[0]:.3e}, {worst[1]:.3e})")
    assert l2.max() <= rel_l2 and mx.max() <= ROW_MAX, f"{what}: row {int(np.argmax(l2))} relL2 = {l2.max():.3e}, row {int(np.argmax(mx))} max = {mx.max():.3e}"


class Plan:
    """the prepared plan of (n, inverse) on the device"""

    def __init__(self, sm, bl, n, inverse, stream=0):
        self.buf = sm.DeviceBuffer(bl.plan_bytes(n))
        bl.prepare(n, self.buf.ptr, inverse, stream=stream)
        self.ptr = self.buf.ptr

    def free(self):
        self.buf.free()


def run(sm, bl, x, inverse=False, front=0, finite=True, launch=None, in_place=False):
    """one launch through the device-pointer API on a copy of x = (batch, n) complex64 that ends where its allocation ends; returns the
    (batch, n) result after checking the guards and (finite) that no NaN of the prefill is left.  front: elements between the output's
    front guard and the output's base; launch(din, dout, n, batch, plan): how to launch, when not on the null stream through the
    mirror; in_place: the input is copied into the guarded buffer, which is input and output"""
    x = np.ascontiguousarray(x)
    assert x.dtype == np.complex64 and x.ndim == 2
    batch, n = x.shape
    plan = Plan(sm, bl, n, inverse)
    dout, pout = rh.guarded(sm, batch * n, 8, front)
    if in_place:
        din, pin = None, pout
        assert sm.lib.smfft_memcpy_h2d(pout, x.ctypes.data, x.nbytes) == 0
    else:
        din = sm.DeviceBuffer.from_host(x)
        assert din.nbytes == x.nbytes
        pin = din.ptr
    try:
        if launch is None:
            bl.launch(pin, pout, n, batch, plan.ptr)
        else:
            launch(pin, pout, n, batch, plan.ptr)
        assert sm.lib.smfft_synchronize() == 0
        return rh.collect(dout, batch * n, np.complex64, front, finite).reshape(batch, n)
    finally:
        for b in (din, dout, plan):
            if b is not None:
                b.free()


def _batch(n, tiles=2, extra=1):
    return tiles * (4096 // bm.fft_size(n)) + extra


# ---- 1: fp64 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 127, 128, 129, 255, 256, 257, 1000, 1021, 1024, 1025, 1536, 2039, 2047, 2048])
def test_against_fp64(sm, bl, n):
    """both sides of every M boundary, primes and powers of two; batch = 2F + 1 (two full tiles and one row), both directions"""
    rng = np.random.default_rng(n)
    x = rh.rand(rng, (_batch(n), n), np.complex64)
    for inverse in (False, True):
        _check_rows(run(sm, bl, x, inverse), _want(x, inverse), f"n={n} inverse={inverse}")


# ---- 2 - 4: exact probes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", SIZES)
def test_probe_impulses(sm, bl, M):
    """row r = an impulse at j in {0, 1, n/2, n - 2, n - 1}, n = the smallest and the largest length of M: X[k] = exp(-+ 2 pi i j k / n),
    every element within ROW_MAX of its value of modulus 1.  This reaches every entry of W and both wrapped halves of b."""
    for n in LENGTHS[M]:
        js = sorted({min(max(j, 0), n - 1) for j in (0, 1, n // 2, n - 2, n - 1)})
        x = np.zeros((len(js), n), np.complex64)
        x[np.arange(len(js)), js] = 1
        k = np.arange(n, dtype=np.int64)
        for inverse in (False, True):
            got = run(sm, bl, x, inverse)
            for r, j in enumerate(js):
                want = np.exp((2j if inverse else -2j) * np.pi * ((j * k) % n) / n)
                err = np.max(np.abs(got[r].astype(np.complex128) - want))
                print(f"M={M} n={n} inverse={inverse} impulse at {j}: max |d| = {err:.3e}")
                assert err <= ROW_MAX, (M, n, inverse, j, err)


@pytest.mark.parametrize("M", SIZES)
def test_probe_tone(sm, bl, M):
    """x[j] = exp(2 pi i k0 j / n), k0 in {0, 1, n/3, n - 1}: n at bin k0 and at most ROW_MAX n in modulus everywhere else (the
    inverse on the conjugate tone likewise).  Chirp phase errors, which random input hides, show here."""
    for n in LENGTHS[M]:
        k0s = sorted({min(max(k0, 0), n - 1) for k0 in (0, 1, n // 3, n - 1)})
        j = np.arange(n, dtype=np.int64)
        tone = np.stack([np.exp(2j * np.pi * ((k0 * j) % n) / n) for k0 in k0s])
        for inverse in (False, True):
            x = (np.conj(tone) if inverse else tone).astype(np.complex64)
            got = run(sm, bl, x, inverse).astype(np.complex128)
            for r, k0 in enumerate(k0s):
                peak = abs(got[r, k0] - n)
                rest = np.abs(np.delete(got[r], k0))
                leak = float(rest.max()) if rest.size else 0.0
                print(f"M={M} n={n} inverse={inverse} k0={k0}: |X[k0] - n| / n = {peak / n:.3e}, max other bin / n = {leak / n:.3e}")
                assert peak <= ROW_MAX * n and leak <= ROW_MAX * n, (M, n, inverse, k0, peak, leak)


@pytest.mark.parametrize("M", ENDS)
def test_probe_rows_are_isolated(sm, bl, M):
    """batch = 3F: one row all NaN, and in a second run one row with a single NaN sample: the poisoned row is NaN in every element and
    every other row keeps the bits of the run without NaN"""
    n = LENGTHS[M][1]
    F = 4096 // M
    rng = np.random.default_rng(50 + M)
    x = rh.rand(rng, (3 * F, n), np.complex64)
    clean = run(sm, bl, x)
    _check_rows(clean, _want(x, False), f"M={M} n={n} clean")
    whole, single = F + F // 2, 2 * F + F // 3
    assert whole != single
    for row, sample in ((whole, None), (single, n // 3)):
        bad = x.copy()
        if sample is None:
            bad[row] = np.nan
        else:
            bad[row, sample] = np.complex64(complex(np.nan, bad[row, sample].imag))
        got = run(sm, bl, bad, finite=False)
        assert np.isnan(got[row]).all(), (M, row, sample, int(np.isnan(got[row]).sum()))
        others = np.arange(3 * F) != row
        assert np.array_equal(rh.bits(got[others]), rh.bits(clean[others])), (M, row, sample)


# ---- 5, 6: the grid -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", SIZES)
def test_grid_is_invisible(sm, bl, M):
    """n = the largest of M, batch = 5F + 1 (six tiles): launch_tuned on 1, 2, 3, 6 and 12288 workgroups gives the bits of launch.  One
    workgroup runs all six tiles with its tables held in registers"""
    n = LENGTHS[M][1]
    rng = np.random.default_rng(60 + M)
    x = rh.rand(rng, (_batch(n, 5), n), np.complex64)
    base = run(sm, bl, x)
    _check_rows(base, _want(x, False), f"M={M} n={n} six tiles")
    for grid in (1, 2, 3, 6, 12288):
        got = run(sm, bl, x, launch=lambda din, dout, n_, batch, plan: bl.launch_tuned(din, dout, n_, batch, plan, grid))
        assert np.array_equal(rh.bits(got), rh.bits(base)), (M, grid)


@pytest.mark.parametrize("n, batch", [(5, 16 * (2 * 12288) + 7), (1025, 2 * 12288 + 1)])
def test_grid_stride_loop(sm, bl, n, batch):
    """more tiles than the grid cap through the plain launch: every workgroup runs two or three tiles, the last tile is partial"""
    F = 4096 // bm.fft_size(n)
    assert GRID_CAP == 12288 and 2 * GRID_CAP < -(-batch // F) <= 3 * GRID_CAP and (F == 1 or batch % F)
    rng = np.random.default_rng(12288 + n)
    x = (rng.standard_normal((batch, n), dtype=np.float32) + 1j * rng.standard_normal((batch, n), dtype=np.float32)).astype(np.complex64)
    _check_rows(run(sm, bl, x), _want(x, False), f"grid-stride n={n} batch={batch}")


# ---- 7, 8: bounds and in-place calls ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", ENDS)
def test_bounds(sm, bl, M):
    """n in {smallest, largest of M}, batch in {1, F - 1, F + 1}, the input ending where its allocation ends, the output base 1 and 3
    elements behind its front guard: nothing in front of or behind the output changes, every output is written, and the bits are those
    at the aligned base, which pass the fp64 bound"""
    F = 4096 // M
    rng = np.random.default_rng(70 + M)
    for n in LENGTHS[M]:
        for batch in sorted({1, max(1, F - 1), F + 1}):
            x = rh.rand(rng, (batch, n), np.complex64)
            for inverse in (False, True):
                base = run(sm, bl, x, inverse)
                _check_rows(base, _want(x, inverse), f"M={M} n={n} batch={batch} inverse={inverse}")
                for front in (1, 3):
                    got = run(sm, bl, x, inverse, front=front)
                    assert np.array_equal(rh.bits(got), rh.bits(base)), f"M={M} n={n} batch={batch} front={front}: the result depends on placement"


@pytest.mark.parametrize("n", [129, 2047])
def test_in_place(sm, bl, n):
    """d_out == d_in, batch = 2F + 1: the bits of the out-of-place run"""
    rng = np.random.default_rng(80 + n)
    x = rh.rand(rng, (_batch(n), n), np.complex64)
    for inverse in (False, True):
        base = run(sm, bl, x, inverse)
        _check_rows(base, _want(x, inverse), f"n={n} inverse={inverse} out of place")
        assert np.array_equal(rh.bits(run(sm, bl, x, inverse, in_place=True)), rh.bits(base)), (n, inverse)


# ---- 9: 64-bit offsets ----------------------------------------------------------------------------------------------------------------
def test_offsets_beyond_two_to_the_31(sm, bl):
    """n = 2047, batch = ceil(2^31 / 2047) + 8 rows in place in one buffer of about 16 GiB, memset to zero, with Gaussian rows at row 0,
    at the row that straddles element 2^31 and at the last two rows: those rows pass the bound, sampled zero rows in between are
    exactly +0, and the guard behind the buffer is intact"""
    n = 2047
    batch = -(-(1 << 31) // n) + 8
    straddle = (1 << 31) // n
    assert straddle * n < (1 << 31) < (straddle + 1) * n and (batch - 2) * n > (1 << 31)
    rows = [0, straddle, batch - 2, batch - 1]
    zeros = [1, straddle // 2, straddle - 1, straddle + 1, batch - 3]
    rng = np.random.default_rng(31)
    x = rh.rand(rng, (len(rows), n), np.complex64)
    total = batch * n
    buf = sm.DeviceBuffer((total + GUARD) * 8)
    plan = Plan(sm, bl, n, False)
    try:
        assert sm.lib.smfft_memset(buf.ptr, 0, total * 8) == 0
        assert sm.lib.smfft_memset(buf.ptr + total * 8, 0x5A, GUARD * 8) == 0
        for i, r in enumerate(rows):
            assert sm.lib.smfft_memcpy_h2d(buf.ptr + r * n * 8, x[i].ctypes.data, n * 8) == 0
        bl.launch(buf.ptr, buf.ptr, n, batch, plan.ptr)
        assert sm.lib.smfft_synchronize() == 0
        guard = np.empty(2 * GUARD, np.uint32)
        assert sm.lib.smfft_memcpy_d2h(guard.ctypes.data, buf.ptr + total * 8, guard.nbytes) == 0
        assert np.all(guard == 0x5A5A5A5A), "the kernel wrote past its buffer"
        got = np.empty((len(rows), n), np.complex64)
        for i, r in enumerate(rows):
            assert sm.lib.smfft_memcpy_d2h(got[i].ctypes.data, buf.ptr + r * n * 8, n * 8) == 0
        _check_rows(got, _want(x, False), "2^31 rows")
        for r in zeros:
            row = np.empty(n, np.complex64)
            assert sm.lib.smfft_memcpy_d2h(row.ctypes.data, buf.ptr + r * n * 8, n * 8) == 0
            words = rh.bits(row)
            print(f"zero row {r}: {int(np.count_nonzero(words))} words that are not +0 ({int(np.count_nonzero(words == 0x80000000))} of them -0)")
            assert not words.any(), f"zero row {r} is not +0 everywhere"
    finally:
        buf.free()
        plan.free()


# ---- 10: the round trip ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 2039])
def test_inverse_round_trip(sm, bl, n):
    """forward, then inverse, divided by n, returns x within 2 ROW_REL_L2 per row"""
    rng = np.random.default_rng(90 + n)
    x = rh.rand(rng, (_batch(n), n), np.complex64)
    back = run(sm, bl, run(sm, bl, x), inverse=True).astype(np.complex128) / n
    l2 = np.linalg.norm(back - x, axis=1) / np.linalg.norm(x.astype(np.complex128), axis=1)
    print(f"n={n}: worst round-trip relL2 = {l2.max():.3e}")
    assert l2.max() <= 2 * ROW_REL_L2, (n, float(l2.max()))


# ---- 11: entry forms ---------------------------------------------------------------------------------------------------------------------
def test_caller_stream(sm, bl):
    """prepare and launch on a stream from hipStreamCreate, then hipStreamSynchronize"""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value
    rng = np.random.default_rng(11)
    for n in (1000, 100):
        x = rh.rand(rng, (37, n), np.complex64)
        for inverse in (False, True):
            def launch(din, dout, n_, batch, plan):
                mine = Plan(sm, bl, n_, inverse, stream=stream.value)       # (the run's own plan goes unused)
                assert sm.lib.smfft_synchronize() == 0                      # the prefill of the output, on the null stream
                bl.launch(din, dout, n_, batch, mine.ptr, stream=stream.value)
                assert hip.hipStreamSynchronize(stream) == 0
                mine.free()
            _check_rows(run(sm, bl, x, inverse, launch=launch), _want(x, inverse), f"stream n={n} inverse={inverse}")
    assert hip.hipStreamDestroy(stream) == 0


def test_benchmark_form_adds_to_the_timer(sm, bl):
    """the library's smfft_bluestein_benchmark adds its milliseconds to a non-zero total and fills the output; so does the mirror's"""
    n = 1536
    rng = np.random.default_rng(12)
    x = rh.rand(rng, (300, n), np.complex64)
    total = ctypes.c_double(1.0)

    def c_form(din, dout, n_, batch, plan):
        assert bl.lib().smfft_bluestein_benchmark(din, dout, n_, batch, plan, ctypes.byref(total)) == 0
        assert total.value > 1.0
    out = run(sm, bl, x, launch=c_form)
    _check_rows(out, _want(x, False), "benchmark form")

    def mirror(din, dout, n_, batch, plan):
        rc, ms = bl.benchmark(din, dout, n_, batch, plan)
        assert rc == 0 and ms > 0.0
    assert np.array_equal(rh.bits(run(sm, bl, x, launch=mirror)), rh.bits(out))


def test_host_round_trip(sm, bl):
    """bluestein.fft on 1-D, 3-D, float64 and real inputs: complex64 of the input's shape, the bits of the device-pointer launch"""
    rng = np.random.default_rng(7)
    x1 = rng.standard_normal(1000) + 1j * rng.standard_normal(1000)                  # 1-D complex128
    got = bl.fft(x1)
    assert got.shape == (1000,) and got.dtype == np.complex64
    assert np.array_equal(rh.bits(got), rh.bits(run(sm, bl, x1.astype(np.complex64)[None])[0]))
    _check_rows(got[None], _want(x1.astype(np.complex64)[None], False), "fft() 1-D")
    x3 = rh.rand(rng, (2, 3, 257), np.complex64)
    for inverse in (False, True):
        got = bl.fft(x3, inverse=inverse)
        assert got.shape == x3.shape and got.dtype == np.complex64
        assert np.array_equal(rh.bits(got.reshape(6, 257)), rh.bits(run(sm, bl, x3.reshape(6, 257), inverse)))
    xr = rng.standard_normal((4, 129))                                               # real float64
    got = bl.fft(xr)
    _check_rows(got, _want(xr.astype(np.float32).astype(np.complex64), False), "fft() real")
    assert got.dtype == np.complex64 and np.array_equal(rh.bits(bl.fft(xr.astype(np.float32))), rh.bits(got))
    assert bl.fft(np.zeros((0, 5), np.complex64)).shape == (0, 5)
    assert ROW_REL_L2 == 1e-6 and ROW_MAX == 5e-6

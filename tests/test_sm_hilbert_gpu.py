"""The Hilbert kernels on an MI355X (smfft_hilbert_launch, smfft_amd.hilbert; one kernel per kind -- 0 H(x), 1 x + i H(x),
2 sqrt(x^2 + H(x)^2) -- and inner length M = n / 2 = 256 ... 4096) against the kernels' chain in fp64, built from NumPy alone
(tools/hilbert_model.py `chain` with float64, which tests/test_sm_hilbert_cpu.py holds to the definition and to scipy.signal.hilbert):
Gaussian rows, rows of very different scales and tones under a large mean at every length; tones at single bins and unit impulses
against their closed forms; a NaN row among others; the place of a row in its batch, the grid and in place against out of place, none
of which may show in the bits; the grid-stride loop; guarded buffers around input and output; 64-bit offsets; a caller's stream, the
benchmark form, tensors and the host round trip.

Every run through `run` goes into an output prefilled with 0xFF (NaN), with a guard of 4096 elements of 0x5A on both sides that must
stay untouched; the input ends where its allocation ends.  Elements are float32, 4 bytes; the analytic kind writes two per sample.

The bound, per row against fp64 and relative to the INPUT row: ||got - want||_2 / ||x||_2 <= ROW_REL_L2 = 1e-6 and
max |got - want| / max |x| <= ROW_MAX = 5e-6, the project's bounds for its fused chains (tests/fir_gpu_harness.py).  Relative to the
input because ||H(x)||_2 <= ||x||_2, and a row dominated by its mean has a small output: the mean passes through the forward transform
and its rounding stays in the other bins.  An fp32 NumPy model of the chain (its transforms in fp64, rounded once: a floor) gave
relL2 <= 6.2e-8 and max <= 9.2e-8 at n = 512 and 8192 (tests/test_sm_hilbert_cpu.py); the kernels measured relL2 <= 3.0e-7 and
max <= 6.0e-7 over all launches of this file when it was written.  The tests print the worst figures they measure per n."""
import ctypes
import os
import sys

import numpy as np
import pytest

from tests import guarded_region
from tests import rows_gpu_harness as rh
from tests.fir_gpu_harness import GRID_CAP, GUARD, ROW_MAX, ROW_REL_L2

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import hilbert_model as hm  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = [512, 1024, 2048, 4096, 8192]
KINDS = [0, 1, 2]
NAMES = {0: "quadrature", 1: "analytic", 2: "envelope"}
WORST = rh.Worst()      # n -> [relL2, max / max]: the worst figures measured in this run
E = 4                       # bytes per element


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def hb():
    from smfft_amd import hilbert
    hilbert.lib()
    return hilbert


def _ffts(n):
    return 8192 // n


def _width(kind):
    """float32 elements of the output per sample"""
    return 2 if kind == 1 else 1


def _check_rows(got, want, x, what):
    """got, want: (batch, n), real or complex; x: the (batch, n) input the bounds are relative to; prints the worst row figures before
    it asserts"""
    n = x.shape[-1]
    d = np.abs(got.astype(np.complex128) - want)
    x = x.astype(np.float64)
    l2 = np.linalg.norm(d, axis=1) / np.maximum(np.linalg.norm(x, axis=1), 1e-300)
    mx = np.max(d, axis=1) / np.maximum(np.max(np.abs(x), axis=1), 1e-300)
    worst = WORST.record(n, l2, mx)
    print(f"{what}: worst row relL2 = {l2.max():.3e}, max |d| / max |x| = {mx.max():.3e}  (n = {n} so far: {worst[0]:.3e}, {worst[1]:.3e})")
    assert l2.max() <= ROW_REL_L2 and mx.max() <= ROW_MAX, \
        f"{what}: row {int(np.argmax(l2))} relL2 = {l2.max():.3e}, row {int(np.argmax(mx))} max = {mx.max():.3e}"


def _shape(flat, batch, n, kind):
    return flat.view(np.complex64).reshape(batch, n) if kind == 1 else flat.reshape(batch, n)


def run(sm, hb, x, kind, finite=True, launch=None, in_place=False):
    """one launch through the device-pointer API on a copy of x = (batch, n) float32.  Out of place: the input ends where its
    allocation ends and the output lies between guards; in place (kinds 0 and 2): the rows lie between guards.  Returns the (batch, n)
    result -- complex64 for the analytic kind -- after checking the guards and (finite) that no NaN of the prefill is left.
    launch(d_in, d_out, n, batch, kind): how to launch, when not on the null stream through the mirror"""
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float32 and x.ndim == 2 and not (in_place and kind == 1)
    batch, n = x.shape
    count = batch * n * _width(kind)
    dout, pout = rh.guarded(sm, count, E)
    din = None
    try:
        if in_place:
            assert sm.lib.smfft_memcpy_h2d(pout, x.ctypes.data, x.nbytes) == 0
            pin = pout
        else:
            din = sm.DeviceBuffer(x.nbytes)
            assert din.nbytes == x.nbytes and sm.lib.smfft_memcpy_h2d(din.ptr, x.ctypes.data, x.nbytes) == 0
            pin = din.ptr
        if launch is None:
            hb.launch_ptr(pin, pout, n, batch, kind)
        else:
            launch(pin, pout, n, batch, kind)
        assert sm.lib.smfft_synchronize() == 0
        return _shape(rh.collect(dout, count, np.float32, finite=finite), batch, n, kind)
    finally:
        for buf in (din, dout):
            if buf is not None:
                buf.free()


def _inputs(n, batch, which):
    """0: Gaussian rows; 1: Gaussian rows whose scale steps from 2^-40 to 2^40 over the batch; 2: a tone of amplitude 1 at a bin of its
    own per row, with a phase, under a mean of 1000"""
    rng = np.random.default_rng(10 * n + which)
    if which == 0:
        return rh.rand(rng, (batch, n))
    if which == 1:
        exps = np.round(np.linspace(-40, 40, batch)).astype(np.int64)
        return np.ldexp(rh.rand(rng, (batch, n)), exps[:, None].astype(np.int32)).astype(np.float32)
    bins = rng.integers(1, n // 2, batch)
    phase = rng.uniform(0, 2 * np.pi, batch)
    return (1000.0 + np.cos(2 * np.pi * np.outer(bins, np.arange(n)) / n + phase[:, None])).astype(np.float32)


# ---- 1: fp64 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", LENGTHS)
def test_against_fp64(sm, hb, n, kind, which):
    """batch = 8192 / n + 1 (one row past a full tile), the three input sets of _inputs; the analytic kind's real part is the input to
    the bit"""
    batch = _ffts(n) + 1
    x = _inputs(n, batch, which)
    got = run(sm, hb, x, kind)
    assert got.shape == (batch, n) and got.dtype == (np.complex64 if kind == 1 else np.float32)
    _check_rows(got, hm.chain(x, kind), x, f"n={n} {NAMES[kind]} inputs {which} batch={batch}")
    if kind == 1:
        assert np.array_equal(rh.bits(got.real), rh.bits(x))


# ---- 2: exact probes ----------------------------------------------------------------------------------------------------------------
def _closed_tone(n, k, phase):
    """(x, H(x)) in fp64 for x[j] = cos(2 pi k j / n + phase): sin(2 pi k j / n + phase) below n / 2, the mirrored bin above, 0 at 0 and
    n / 2"""
    j = np.arange(n)
    x = np.cos(2 * np.pi * k * j / n + phase)
    if k in (0, n // 2):
        return x, np.zeros(n)
    if k < n // 2:
        return x, np.sin(2 * np.pi * k * j / n + phase)
    return x, np.sin(2 * np.pi * (n - k) * j / n - phase)


def _closed_impulse(n, j0):
    """H(e_j0)[j] = (2 / n) cot(pi (j - j0) / n) at odd j - j0, 0 at even"""
    d = np.arange(n) - j0
    h = np.zeros(n)
    odd = d % 2 != 0
    h[odd] = 2.0 / n / np.tan(np.pi * d[odd] / n)
    return h


def _of_kind(x, h, kind):
    return h if kind == 0 else x + 1j * h if kind == 1 else np.sqrt(x * x + h * h)


@pytest.mark.parametrize("n", [512, 4096])
def test_probe_tones_and_impulses(sm, hb, n):
    """a tone cos(2 pi k j / n + 0.3) at every bin k (n = 512) or at k in {0, 1, M - 1, M, M + 1, n - 1} and 16 random bins (n = 4096,
    M = n / 2), and a unit impulse at each of j in {0, 1, n / 2, n - 1}, against the closed forms (which the fp64 definition meets
    within 1e-10), for the three kinds.  The tones are rounded to float32 before the launch: that is 2^-25 of the bound's scale per
    sample, inside the bounds.  A wrong sign of s[k], a wrong partner or a bin 0 / n / 2 that is not zeroed shows as an error of order 1"""
    M = n // 2
    rng = np.random.default_rng(25 + n)
    bins = list(range(n)) if n == 512 else [0, 1, M - 1, M, M + 1, n - 1] + sorted(rng.choice(np.arange(2, n - 1), 16, replace=False).tolist())
    pairs = [_closed_tone(n, k, 0.3) for k in bins]
    places = [0, 1, n // 2, n - 1]
    for j0 in places:
        e = np.zeros(n)
        e[j0] = 1.0
        pairs.append((e, _closed_impulse(n, j0)))
    x64, h64 = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    assert np.abs(hm.direct(x64) - h64).max() <= 1e-10
    x = x64.astype(np.float32)
    for kind in KINDS:
        got = run(sm, hb, x, kind)
        want = _of_kind(x.astype(np.float64), h64, kind)
        _check_rows(got[:len(bins)], want[:len(bins)], x[:len(bins)], f"n={n} {NAMES[kind]} tones at {len(bins)} bins")
        _check_rows(got[len(bins):], want[len(bins):], x[len(bins):], f"n={n} {NAMES[kind]} impulses at {places}")


# ---- 3: isolation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_probe_rows_are_isolated(sm, hb, n):
    """batch = 2 (8192 / n) + 1, one row all NaN, then one row with a single +Inf sample: that row is not finite (a NaN or an Inf in every element or
    nearly: every output is a sum over the whole row) and every other row keeps the bits of the clean run"""
    F = _ffts(n)
    batch = 2 * F + 1
    x = rh.rand(np.random.default_rng(30 + n), (batch, n))
    row = F + F // 2
    for kind in KINDS:
        clean = run(sm, hb, x, kind)
        _check_rows(clean, hm.chain(x, kind), x, f"n={n} {NAMES[kind]} clean")
        for case in ("all NaN", "one +Inf"):
            bad = x.copy()
            if case == "all NaN":
                bad[row] = np.nan
            else:
                bad[row, n // 3] = np.inf
            got = run(sm, hb, bad, kind, finite=False)
            part = got[row].imag if kind == 1 else got[row]                # (the analytic kind's real part is the input itself)
            print(f"n={n} {NAMES[kind]} {case}: {int(np.isfinite(part).sum())} of {n} outputs of the row are finite")
            assert not np.isfinite(part).all(), (n, kind, case)
            others = np.arange(batch) != row
            assert np.array_equal(rh.bits(got[others]), rh.bits(clean[others])), (n, kind, case)


@pytest.mark.parametrize("n", LENGTHS)
def test_position_grid_and_in_place_are_invisible(sm, hb, n):
    """batch = 3 (8192 / n) + 1 among other Gaussian rows: one row alone, at row 0, at the last slot of the first tile, in the middle
    and as the ragged last row gives the same bits; launch_tuned on 1 and 3 workgroups gives the bits of the default launch; and so
    does the launch with d_out == d_in, between guards, for kinds 0 and 2 -- also on one workgroup, which then runs every tile"""
    F = _ffts(n)
    batch = 3 * F + 1
    rng = np.random.default_rng(40 + n)
    probe = rh.rand(rng, (1, n))
    x = rh.rand(rng, (batch, n))
    places = sorted({0, F - 1, F + F // 2, batch - 1})
    x[places] = probe[0]
    for kind in KINDS:
        alone = run(sm, hb, probe, kind)
        _check_rows(alone, hm.chain(probe, kind), probe, f"n={n} {NAMES[kind]} alone")
        base = run(sm, hb, x, kind)
        for r in places:
            assert np.array_equal(rh.bits(base[r]), rh.bits(alone[0])), (n, kind, r)
        for grid in (1, 3):
            got = run(sm, hb, x, kind, launch=lambda i, o, nn, b, k: hb.launch_tuned(i, o, nn, b, grid, k))
            assert np.array_equal(rh.bits(got), rh.bits(base)), (n, kind, grid)
        if kind != 1:
            assert np.array_equal(rh.bits(run(sm, hb, x, kind, in_place=True)), rh.bits(base)), (n, kind, "in place")
            got = run(sm, hb, x, kind, in_place=True, launch=lambda i, o, nn, b, k: hb.launch_tuned(i, o, nn, b, 1, k))
            assert np.array_equal(rh.bits(got), rh.bits(base)), (n, kind, "in place, one workgroup")


# ---- 4: the grid-stride loop ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_grid_stride_loop(sm, hb, kind):
    """n = 512, batch = 16 (2 * 12288) + 7 through the plain launch: more tiles than the grid cap, every workgroup runs two or three
    tiles of sixteen rows.  Row r holds block[r % 4096] of 4096 Gaussian rows; the rows of the first tile, around every multiple of
    the cap, the last ones and every 997th are fetched and held to the fp64 chain; the guard behind the output is intact"""
    n, F, W = 512, 16, _width(kind)
    batch = F * (2 * GRID_CAP) + 7
    assert GRID_CAP == 12288 and GRID_CAP < -(-batch // F) <= 3 * GRID_CAP and batch % F
    block = rh.rand(np.random.default_rng(50 + kind), (4096, n))
    want = hm.chain(block, kind)
    din, dout = sm.DeviceBuffer(batch * n * E), sm.DeviceBuffer((batch * n * W + GUARD) * E)
    try:
        for first in range(0, batch, 4096):
            rows = min(4096, batch - first)
            assert sm.lib.smfft_memcpy_h2d(din.ptr + first * n * E, block.ctypes.data, rows * n * E) == 0
        assert sm.lib.smfft_memset(dout.ptr, 0xFF, batch * n * W * E) == 0
        assert sm.lib.smfft_memset(dout.ptr + batch * n * W * E, 0x5A, GUARD * E) == 0
        hb.launch_ptr(din.ptr, dout.ptr, n, batch, kind)
        assert sm.lib.smfft_synchronize() == 0
        guard = np.empty(GUARD, np.uint32)
        assert sm.lib.smfft_memcpy_d2h(guard.ctypes.data, dout.ptr + batch * n * W * E, guard.nbytes) == 0
        assert np.all(guard == 0x5A5A5A5A), "the kernel wrote past its output"
        picked = set(range(F)) | set(range(batch - F - 7, batch)) | set(range(0, batch, 997))
        for c in (1, 2):
            picked |= set(range(c * GRID_CAP * F - 2, c * GRID_CAP * F + 2))
        picked = sorted(picked)
        got = np.empty((len(picked), n * W), np.float32)
        for i, r in enumerate(picked):
            assert sm.lib.smfft_memcpy_d2h(got[i].ctypes.data, dout.ptr + r * n * W * E, n * W * E) == 0
        assert np.all(np.isfinite(got)), "outputs left unwritten"
        idx = np.array(picked) % 4096
        _check_rows(_shape(got.reshape(-1), len(picked), n, kind), want[idx], block[idx], f"grid-stride n={n} batch={batch} {NAMES[kind]}, {len(picked)} rows")
    finally:
        din.free()
        dout.free()


# ---- 5: bounds ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, batch", [(512, 17), (8192, 1)])
def test_bounds(sm, hb, n, batch):
    """input and output each inside a poisoned allocation with 128 KiB of guard on both sides (tests/guarded_region.py), the three
    kinds: the input and everything around it are unchanged, nothing around the output's elements is written, every one of them is, and
    the bits are those of the plain run, which passes the fp64 bound.  (A read outside the input would pick up the poison, a NaN, and
    show in the result.)"""
    x = rh.rand(np.random.default_rng(60 + n), (batch, n))
    for kind in KINDS:
        base = run(sm, hb, x, kind)
        _check_rows(base, hm.chain(x, kind), x, f"n={n} batch={batch} {NAMES[kind]}")
        rin = guarded_region.Region(sm, x.view(np.uint8).reshape(-1), 0, align=4)
        rout = guarded_region.Region(sm, guarded_region.poison(x.nbytes * _width(kind)), 8 if kind == 1 else 4, align=4)
        try:
            hb.launch_ptr(rin.ptr, rout.ptr, n, batch, kind)
            assert sm.lib.smfft_synchronize() == 0
            rin.outside_unchanged(whole=True)
            got = rout.outside_unchanged(whole=False).view(np.float32)
            assert np.array_equal(rh.bits(got), rh.bits(base).reshape(-1)), (n, batch, kind)
        finally:
            rin.buf.free()
            rout.buf.free()


def test_adjacent_buffers_are_served(sm, hb):
    """n = 1024, batch = 9: input and output in one allocation, the output right behind the input and right in front of it -- the
    nearest ranges that the overlap check must not refuse -- give the bits of the plain run, and the input is unchanged"""
    n, batch = 1024, 9
    x = rh.rand(np.random.default_rng(65), (batch, n))
    for kind in KINDS:
        base = run(sm, hb, x, kind)
        count = batch * n * _width(kind)
        buf = sm.DeviceBuffer((batch * n + count) * E)
        try:
            for pin, pout in ((buf.ptr, buf.ptr + batch * n * E), (buf.ptr + count * E, buf.ptr)):
                assert sm.lib.smfft_memset(buf.ptr, 0xFF, buf.nbytes) == 0
                assert sm.lib.smfft_memcpy_h2d(pin, x.ctypes.data, x.nbytes) == 0
                hb.launch_ptr(pin, pout, n, batch, kind)
                assert sm.lib.smfft_synchronize() == 0
                got, back = np.empty(count, np.float32), np.empty_like(x)
                assert sm.lib.smfft_memcpy_d2h(got.ctypes.data, pout, got.nbytes) == 0
                assert sm.lib.smfft_memcpy_d2h(back.ctypes.data, pin, back.nbytes) == 0
                assert np.array_equal(rh.bits(got), rh.bits(base).reshape(-1)) and np.array_equal(rh.bits(back), rh.bits(x)), kind
        finally:
            buf.free()


# ---- 6: 64-bit offsets ----------------------------------------------------------------------------------------------------------------
def test_offsets_beyond_two_to_the_31(sm, hb):
    """n = 8192, kind 0, batch = 2^31 / 8192 + 8 rows, 8 GiB, in place: the rows are memset to zero, with Gaussian rows at the first
    two, at those on both sides of byte 2^31, of byte 2^32 and of element 2^31, and at the last two.  Those rows pass the bound,
    sampled zero rows give zeros, and the guard behind the buffer is intact"""
    n, kind = 8192, 0
    batch = (1 << 31) // n + 8
    assert (batch - 8) * n == 1 << 31
    rows = [0, 1, (1 << 29) // n - 1, (1 << 29) // n, (1 << 30) // n - 1, (1 << 30) // n, (1 << 31) // n - 1, (1 << 31) // n, batch - 2, batch - 1]
    zeros = [2, (1 << 29) // n + 1, (1 << 31) // n - 2, (1 << 31) // n + 1, batch - 3]
    x = rh.rand(np.random.default_rng(70), (len(rows), n))
    want = hm.chain(x, kind)
    buf = sm.DeviceBuffer((batch * n + GUARD) * E)
    try:
        assert sm.lib.smfft_memset(buf.ptr, 0, batch * n * E) == 0
        assert sm.lib.smfft_memset(buf.ptr + batch * n * E, 0x5A, GUARD * E) == 0
        for i, r in enumerate(rows):
            assert sm.lib.smfft_memcpy_h2d(buf.ptr + r * n * E, x[i].ctypes.data, n * E) == 0
        hb.launch_ptr(buf.ptr, buf.ptr, n, batch, kind)
        assert sm.lib.smfft_synchronize() == 0
        guard = np.empty(GUARD, np.uint32)
        assert sm.lib.smfft_memcpy_d2h(guard.ctypes.data, buf.ptr + batch * n * E, guard.nbytes) == 0
        assert np.all(guard == 0x5A5A5A5A), "the kernel wrote past its buffer"
        got = np.empty((len(rows), n), np.float32)
        for i, r in enumerate(rows):
            assert sm.lib.smfft_memcpy_d2h(got[i].ctypes.data, buf.ptr + r * n * E, n * E) == 0
        _check_rows(got, want, x, "2^31 rows quadrature")
        row = np.empty(n, np.float32)
        for r in zeros:
            assert sm.lib.smfft_memcpy_d2h(row.ctypes.data, buf.ptr + r * n * E, n * E) == 0
            assert not row.any(), f"zero row {r} is not zero everywhere"
    finally:
        buf.free()


# ---- 7: entry forms ---------------------------------------------------------------------------------------------------------------------
def test_caller_stream(sm, hb):
    """launch on a stream from hipStreamCreate, then hipStreamSynchronize"""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value
    rng = np.random.default_rng(11)
    for n, kind in ((1024, 1), (4096, 2)):
        x = rh.rand(rng, (37, n))

        def launch(din, dout, nn, batch, k):
            assert sm.lib.smfft_synchronize() == 0                              # the prefill of the output, on the null stream
            hb.launch_ptr(din, dout, nn, batch, k, stream=stream.value)
            assert hip.hipStreamSynchronize(stream) == 0
        _check_rows(run(sm, hb, x, kind, launch=launch), hm.chain(x, kind), x, f"stream n={n} {NAMES[kind]}")
    assert hip.hipStreamDestroy(stream) == 0


def test_benchmark_form_adds_to_the_timer(sm, hb):
    """the library's smfft_hilbert_benchmark adds its milliseconds to a non-zero total and fills the output; so does the mirror's"""
    n = 2048
    x = rh.rand(np.random.default_rng(12), (300, n))
    total = ctypes.c_double(1.0)

    def c_form(din, dout, nn, batch, k):
        assert hb.lib().smfft_hilbert_benchmark(din, dout, nn, batch, k, ctypes.byref(total)) == 0
        assert total.value > 1.0
    out = run(sm, hb, x, 0, launch=c_form)
    _check_rows(out, hm.chain(x, 0), x, "benchmark form")

    def mirror(din, dout, nn, batch, k):
        status, ms = hb.benchmark(din, dout, nn, batch, k)
        assert status == 0 and ms > 0.0
    assert np.array_equal(rh.bits(run(sm, hb, x, 0, launch=mirror)), rh.bits(out))


def test_host_round_trip(sm, hb):
    """hilbert / analytic / envelope on 1-D, 3-D and float64 host arrays: float32 (complex64) of the input's shape with the bits of the
    device-pointer launch; a CPU tensor gives a CPU tensor; an empty batch returns an empty array; unsupported lengths raise ValueError"""
    import torch
    rng = np.random.default_rng(7)
    x1 = rng.standard_normal(1024)                                                  # 1-D float64
    got = hb.hilbert(x1)
    assert got.shape == (1024,) and got.dtype == np.float32
    assert np.array_equal(rh.bits(got), rh.bits(run(sm, hb, x1.astype(np.float32)[None], 0)[0]))
    _check_rows(got[None], hm.chain(x1.astype(np.float32)[None], 0), x1[None], "hilbert() 1-D")
    x3 = rh.rand(rng, (2, 3, 512))
    for kind, fn, dtype in ((0, hb.hilbert, np.float32), (1, hb.analytic, np.complex64), (2, hb.envelope, np.float32)):
        got = fn(x3)
        assert got.shape == x3.shape and got.dtype == dtype
        assert np.array_equal(rh.bits(got.reshape(6, 512)), rh.bits(run(sm, hb, x3.reshape(6, 512), kind)))
    a = hb.analytic(torch.from_numpy(x3))
    assert isinstance(a, torch.Tensor) and not a.is_cuda and a.dtype == torch.complex64 and a.shape == x3.shape
    assert np.array_equal(rh.bits(a.numpy()), rh.bits(hb.analytic(x3))) and np.array_equal(rh.bits(a.numpy().real), rh.bits(x3))
    for fn, dtype in ((hb.hilbert, np.float32), (hb.analytic, np.complex64)):
        empty = fn(np.zeros((0, 512), np.float32))
        assert empty.shape == (0, 512) and empty.dtype == dtype
    for bad in (np.zeros(256), np.zeros(500), np.zeros((2, 16384))):
        with pytest.raises(ValueError):
            hb.envelope(bad)
    assert ROW_REL_L2 == 1e-6 and ROW_MAX == 5e-6


def test_tensors_on_the_device(sm, hb):
    """launch / hilbert / analytic / envelope on float32 torch tensors on the device: a new tensor, a given one (complex64 for the
    analytic kind), and x itself (in place, kinds 0 and 2) hold the bits of the device-pointer launch; a tensor that is not contiguous
    float32, an out of the wrong dtype or shape and the analytic kind in place are refused"""
    import torch
    rng = np.random.default_rng(8)
    x = rh.rand(rng, (5, 3, 2048))
    t = torch.from_numpy(x).cuda()
    for kind, fn in ((0, hb.hilbert), (1, hb.analytic), (2, hb.envelope)):
        dtype = torch.complex64 if kind == 1 else torch.float32
        want = run(sm, hb, x.reshape(15, 2048), kind).reshape(x.shape)
        got = fn(t)
        assert got.shape == t.shape and got.dtype == dtype and got.is_cuda and got.data_ptr() != t.data_ptr()
        torch.cuda.synchronize()
        assert np.array_equal(rh.bits(got.cpu().numpy()), rh.bits(want)), kind
        out = torch.full(t.shape, float("nan"), dtype=dtype, device="cuda")
        assert hb.launch(t, out, kind=kind) is out
        torch.cuda.synchronize()
        assert np.array_equal(rh.bits(out.cpu().numpy()), rh.bits(want)), kind
        if kind != 1:
            work = t.clone()
            assert hb.launch(work, work, kind=kind) is work
            torch.cuda.synchronize()
            assert np.array_equal(rh.bits(work.cpu().numpy()), rh.bits(want)), kind
    with pytest.raises(TypeError):
        hb.launch(t.double())
    with pytest.raises(ValueError):
        hb.launch(t[:, :, ::2])
    with pytest.raises(ValueError):
        hb.launch(t, torch.empty(5, 3, 1024, device="cuda"))
    with pytest.raises(TypeError):
        hb.launch(t, torch.empty_like(t), kind=hb.ANALYTIC)
    with pytest.raises(TypeError):
        hb.launch(t, torch.empty(t.shape, dtype=torch.complex64, device="cuda"), kind=hb.ENVELOPE)

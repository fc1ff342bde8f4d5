"""The DCT / DST kernels on an MI355X (smfft_dct_launch, smfft_amd.dct; the type II and the type III kernel per inner length
M = n / 2 = 256 ... 4096) against the kernels' chain in fp64, built from NumPy alone (tools/dct_model.py `chain` with float64, which
tests/test_sm_dct_cpu.py holds to the sums of the definition at n = 512): Gaussian rows at every length, for the four transforms, as a
single row, with a ragged last tile and one row past a full tile; unit impulses at the ends and the middle of a row against the cosine
and sine columns of the definition; the round trip through type II and type III; a NaN row among others; the place of a row in its
batch, the grid and in place against out of place, none of which may show in the bits; the grid-stride loop; guarded buffers around
input and output; 64-bit offsets; a caller's stream, the benchmark form, tensors and the host round trip.

Every run through `run` goes into an output prefilled with 0xFF (NaN), with a guard of 4096 elements of 0x5A on both sides that must
stay untouched; the input ends where its allocation ends.  Elements are float32: 4 bytes.

The bound, per row against fp64: ||d||_2 / ||want||_2 <= ROW_REL_L2 = 1e-6 and max |d| / max |want| <= ROW_MAX = 5e-6, the project's
bounds for its fused chains (tests/fir_gpu_harness.py, tests/test_sm_rowconv_real_gpu.py).  An fp32 NumPy model of the chain gave
relL2 <= 7e-8 and max <= 1.3e-7 at n = 512 and 8192 (tests/test_sm_dct_cpu.py); the kernels measured relL2 <= 1.6e-7 and max <= 3.7e-7
on single launches when this was written.  The round trip is held to twice the bounds: two launches (measured 2.4e-7 / 3.4e-7).  The
tests print the worst figures they measure per n.

The file's name makes it collect behind every older GPU test file but the two of the row-pair convolutions, which follow it unchanged."""
import ctypes
import os
import sys

import numpy as np
import pytest

from tests import guarded_region
from tests import rows_gpu_harness as rh
from tests.fir_gpu_harness import GRID_CAP, GUARD, ROW_MAX, ROW_REL_L2

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import dct_model as dm  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = [512, 1024, 2048, 4096, 8192]
TRANSFORMS = [(2, False), (3, False), (2, True), (3, True)]       # (type, sine)
WORST = rh.Worst()      # n -> [relL2, max / max]: the worst figures measured in this run
E = 4                       # bytes per element


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def dc():
    from smfft_amd import dct
    dct.lib()
    return dct


def _name(type, sine):
    return f"{'DST' if sine else 'DCT'}-{'II' if type == 2 else 'III'}"


def _ffts(n):
    return 8192 // n


def _check_rows(got, want, n, what, factor=1.0):
    """got, want: (batch, n); prints the worst row figures before it asserts"""
    d = got.astype(np.float64) - want
    l2 = np.linalg.norm(d, axis=1) / np.maximum(np.linalg.norm(want, axis=1), 1e-300)
    mx = np.max(np.abs(d), axis=1) / np.maximum(np.max(np.abs(want), axis=1), 1e-300)
    worst = WORST.record(n, l2, mx)
    print(f"{what}: worst row relL2 = {l2.max():.3e}, max |d| / max |want| = {mx.max():.3e}  (n = {n} so far: {worst[0]:.3e}, {worst[1]:.3e})")
    assert l2.max() <= factor * ROW_REL_L2 and mx.max() <= factor * ROW_MAX, \
        f"{what}: row {int(np.argmax(l2))} relL2 = {l2.max():.3e}, row {int(np.argmax(mx))} max = {mx.max():.3e}"


def run(sm, dc, x, type, sine, finite=True, launch=None, in_place=False):
    """one launch through the device-pointer API on a copy of x = (batch, n) float32.  Out of place: the input ends where its
    allocation ends and the output lies between guards; in place: the rows lie between guards.  Returns the (batch, n) result after
    checking the guards and (finite) that no NaN of the prefill is left.  launch(d_in, d_out, n, batch, type, sine): how to launch,
    when not on the null stream through the mirror"""
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    batch, n = x.shape
    dout, pout = rh.guarded(sm, batch * n, E)
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
            dc.launch_ptr(pin, pout, n, batch, type, sine)
        else:
            launch(pin, pout, n, batch, type, sine)
        assert sm.lib.smfft_synchronize() == 0
        return rh.collect(dout, batch * n, np.float32, finite=finite).reshape(batch, n)
    finally:
        for buf in (din, dout):
            if buf is not None:
                buf.free()


# ---- 1: fp64 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("type, sine", TRANSFORMS)
@pytest.mark.parametrize("n", LENGTHS)
def test_against_fp64(sm, dc, n, type, sine, which):
    """batch = 1 (a single row), 17 (a ragged last tile at sixteen rows per workgroup, several tiles above) and 8192 / n + 1 (one row
    past a full tile)"""
    batch = (1, 17, _ffts(n) + 1)[which]
    x = rh.rand(np.random.default_rng(10 * n + batch), (batch, n))
    got = run(sm, dc, x, type, sine)
    assert got.shape == (batch, n) and got.dtype == np.float32
    _check_rows(got, dm.chain(x, type, sine), n, f"n={n} {_name(type, sine)} batch={batch}")


# ---- 2: exact probes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [512, 4096])
def test_probe_impulses(sm, dc, n):
    """rows e_0, e_1, e_{n/2-1}, e_{n/2}, e_{n-1}, as x for type II and as X for type III: the cosine or sine column of the definition
    (the fp64 sums themselves, tools/dct_model.py `direct`) within the row bounds.  A wrong index in the permutation or in the
    X[n - k] store moves or mirrors the column"""
    js = [0, 1, n // 2 - 1, n // 2, n - 1]
    x = np.zeros((len(js), n), np.float32)
    x[np.arange(len(js)), js] = 1
    for type, sine in TRANSFORMS:
        want = dm.direct(x, type, sine)
        assert np.abs(want).max() <= 2.0 + 1e-12 and np.abs(want).max() >= 1.0
        _check_rows(run(sm, dc, x, type, sine), want, n, f"n={n} {_name(type, sine)} impulses at {js}")


@pytest.mark.parametrize("n", LENGTHS)
def test_round_trip(sm, dc, n):
    """DCT-III(DCT-II(x)) / (2n) and DST-III(DST-II(x)) / (2n) return x within twice the row bounds (two launches), batch = 8192 / n + 1"""
    x = rh.rand(np.random.default_rng(20 + n), (_ffts(n) + 1, n))
    for sine in (False, True):
        forward = run(sm, dc, x, 2, sine)
        back = run(sm, dc, forward, 3, sine)
        _check_rows(back.astype(np.float64) / (2 * n), x.astype(np.float64), n, f"n={n} {'DST' if sine else 'DCT'} round trip", factor=2.0)


# ---- 3: isolation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_probe_rows_are_isolated(sm, dc, n):
    """batch = 2 (8192 / n) + 1, one row all NaN, then one row with a single +Inf sample: that row has no finite output (a NaN or an Inf
    in every element or nearly: each output is a sum over the whole row) and every other row keeps the bits of the clean run"""
    F = _ffts(n)
    batch = 2 * F + 1
    x = rh.rand(np.random.default_rng(30 + n), (batch, n))
    row = F + F // 2
    for type, sine in TRANSFORMS:
        clean = run(sm, dc, x, type, sine)
        _check_rows(clean, dm.chain(x, type, sine), n, f"n={n} {_name(type, sine)} clean")
        for case in ("all NaN", "one +Inf"):
            bad = x.copy()
            if case == "all NaN":
                bad[row] = np.nan
            else:
                bad[row, n // 3] = np.inf
            got = run(sm, dc, bad, type, sine, finite=False)
            assert not np.isfinite(got[row]).all(), (n, type, sine, case)
            others = np.arange(batch) != row
            assert np.array_equal(rh.bits(got[others]), rh.bits(clean[others])), (n, type, sine, case)


@pytest.mark.parametrize("n", LENGTHS)
def test_position_grid_and_in_place_are_invisible(sm, dc, n):
    """batch = 3 (8192 / n) + 1 among other Gaussian rows: one row alone, at row 0, at the last slot of the first tile, in the middle
    and as the ragged last row gives the same bits; launch_tuned on 1 and 3 workgroups gives the bits of the default launch; and so
    does the launch with d_out == d_in, between guards.  All four transforms"""
    F = _ffts(n)
    batch = 3 * F + 1
    rng = np.random.default_rng(40 + n)
    probe = rh.rand(rng, (1, n))
    x = rh.rand(rng, (batch, n))
    places = sorted({0, F - 1, F + F // 2, batch - 1})
    x[places] = probe[0]
    for type, sine in TRANSFORMS:
        alone = run(sm, dc, probe, type, sine)
        _check_rows(alone, dm.chain(probe, type, sine), n, f"n={n} {_name(type, sine)} alone")
        base = run(sm, dc, x, type, sine)
        for r in places:
            assert np.array_equal(rh.bits(base[r]), rh.bits(alone[0])), (n, type, sine, r)
        for grid in (1, 3):
            got = run(sm, dc, x, type, sine, launch=lambda i, o, nn, b, t, s: dc.launch_tuned(i, o, nn, b, grid, t, s))
            assert np.array_equal(rh.bits(got), rh.bits(base)), (n, type, sine, grid)
        assert np.array_equal(rh.bits(run(sm, dc, x, type, sine, in_place=True)), rh.bits(base)), (n, type, sine, "in place")
        got = run(sm, dc, x, type, sine, in_place=True, launch=lambda i, o, nn, b, t, s: dc.launch_tuned(i, o, nn, b, 1, t, s))
        assert np.array_equal(rh.bits(got), rh.bits(base)), (n, type, sine, "in place, one workgroup")


# ---- 4: the grid-stride loop ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("type, sine", [(2, False), (3, True)])
def test_grid_stride_loop(sm, dc, type, sine):
    """n = 512, batch = 16 (2 * 12288) + 7 through the plain launch: more tiles than the grid cap, every workgroup runs two or three
    tiles of sixteen rows.  Row r holds block[r % 4096] of 4096 Gaussian rows; the rows of the first tile, around every multiple of
    the cap, the last ones and every 997th are fetched and held to the fp64 chain"""
    n, F = 512, 16
    batch = F * (2 * GRID_CAP) + 7
    assert GRID_CAP == 12288 and GRID_CAP < -(-batch // F) <= 3 * GRID_CAP and batch % F
    block = rh.rand(np.random.default_rng(50 + type), (4096, n))
    want = dm.chain(block, type, sine)
    din, dout = sm.DeviceBuffer(batch * n * E), sm.DeviceBuffer((batch * n + GUARD) * E)
    try:
        for first in range(0, batch, 4096):
            rows = min(4096, batch - first)
            assert sm.lib.smfft_memcpy_h2d(din.ptr + first * n * E, block.ctypes.data, rows * n * E) == 0
        assert sm.lib.smfft_memset(dout.ptr, 0xFF, batch * n * E) == 0
        assert sm.lib.smfft_memset(dout.ptr + batch * n * E, 0x5A, GUARD * E) == 0
        dc.launch_ptr(din.ptr, dout.ptr, n, batch, type, sine)
        assert sm.lib.smfft_synchronize() == 0
        guard = np.empty(GUARD, np.uint32)
        assert sm.lib.smfft_memcpy_d2h(guard.ctypes.data, dout.ptr + batch * n * E, guard.nbytes) == 0
        assert np.all(guard == 0x5A5A5A5A), "the kernel wrote past its output"
        picked = set(range(F)) | set(range(batch - F - 7, batch)) | set(range(0, batch, 997))
        for c in (1, 2):
            picked |= set(range(c * GRID_CAP * F - 2, c * GRID_CAP * F + 2))
        picked = sorted(picked)
        got = np.empty((len(picked), n), np.float32)
        for i, r in enumerate(picked):
            assert sm.lib.smfft_memcpy_d2h(got[i].ctypes.data, dout.ptr + r * n * E, n * E) == 0
        assert np.all(np.isfinite(got)), "outputs left unwritten"
        _check_rows(got, want[np.array(picked) % 4096], n, f"grid-stride n={n} batch={batch} {_name(type, sine)}, {len(picked)} rows")
    finally:
        din.free()
        dout.free()


# ---- 5: bounds ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, batch", [(512, 17), (8192, 1)])
def test_bounds(sm, dc, n, batch):
    """input and output each inside a poisoned allocation with 128 KiB of guard on both sides (tests/guarded_region.py), the four
    transforms: the input and everything around it are unchanged, nothing around the batch * n output floats is written, every output
    is, and the bits are those of the plain run, which passes the fp64 bound.  (A read outside the input would pick up the poison, a
    NaN, and show in the result.)"""
    x = rh.rand(np.random.default_rng(60 + n), (batch, n))
    for type, sine in TRANSFORMS:
        base = run(sm, dc, x, type, sine)
        _check_rows(base, dm.chain(x, type, sine), n, f"n={n} batch={batch} {_name(type, sine)}")
        rin = guarded_region.Region(sm, x.view(np.uint8).reshape(-1), 0, align=4)
        rout = guarded_region.Region(sm, guarded_region.poison(x.nbytes), 4, align=4)
        try:
            dc.launch_ptr(rin.ptr, rout.ptr, n, batch, type, sine)
            assert sm.lib.smfft_synchronize() == 0
            rin.outside_unchanged(whole=True)
            got = rout.outside_unchanged(whole=False).view(np.float32).reshape(batch, n)
            assert np.array_equal(rh.bits(got), rh.bits(base)), (n, batch, type, sine)
        finally:
            rin.buf.free()
            rout.buf.free()


# ---- 6: 64-bit offsets ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("type, sine", TRANSFORMS)
def test_offsets_beyond_two_to_the_31(sm, dc, type, sine):
    """n = 8192, batch = 2^31 / 8192 + 8 rows, 8 GiB, in place: the rows are memset to zero, with Gaussian rows at the first two, at
    those on both sides of byte 2^31, of byte 2^32 and of element 2^31, and at the last two.  Those rows pass the bound, sampled zero
    rows give zeros, and the guard behind the buffer is intact"""
    n = 8192
    batch = (1 << 31) // n + 8
    assert (batch - 8) * n == 1 << 31
    rows = [0, 1, (1 << 29) // n - 1, (1 << 29) // n, (1 << 30) // n - 1, (1 << 30) // n, (1 << 31) // n - 1, (1 << 31) // n, batch - 2, batch - 1]
    zeros = [2, (1 << 29) // n + 1, (1 << 31) // n - 2, (1 << 31) // n + 1, batch - 3]
    x = rh.rand(np.random.default_rng(70 + type), (len(rows), n))
    want = dm.chain(x, type, sine)
    buf = sm.DeviceBuffer((batch * n + GUARD) * E)
    try:
        assert sm.lib.smfft_memset(buf.ptr, 0, batch * n * E) == 0
        assert sm.lib.smfft_memset(buf.ptr + batch * n * E, 0x5A, GUARD * E) == 0
        for i, r in enumerate(rows):
            assert sm.lib.smfft_memcpy_h2d(buf.ptr + r * n * E, x[i].ctypes.data, n * E) == 0
        dc.launch_ptr(buf.ptr, buf.ptr, n, batch, type, sine)
        assert sm.lib.smfft_synchronize() == 0
        guard = np.empty(GUARD, np.uint32)
        assert sm.lib.smfft_memcpy_d2h(guard.ctypes.data, buf.ptr + batch * n * E, guard.nbytes) == 0
        assert np.all(guard == 0x5A5A5A5A), "the kernel wrote past its buffer"
        got = np.empty((len(rows), n), np.float32)
        for i, r in enumerate(rows):
            assert sm.lib.smfft_memcpy_d2h(got[i].ctypes.data, buf.ptr + r * n * E, n * E) == 0
        _check_rows(got, want, n, f"2^31 rows {_name(type, sine)}")
        row = np.empty(n, np.float32)
        for r in zeros:
            assert sm.lib.smfft_memcpy_d2h(row.ctypes.data, buf.ptr + r * n * E, n * E) == 0
            assert not row.any(), f"zero row {r} is not zero everywhere"
    finally:
        buf.free()


# ---- 7: entry forms ---------------------------------------------------------------------------------------------------------------------
def test_caller_stream(sm, dc):
    """launch on a stream from hipStreamCreate, then hipStreamSynchronize"""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value
    rng = np.random.default_rng(11)
    for n, type, sine in ((1024, 2, True), (4096, 3, False)):
        x = rh.rand(rng, (37, n))

        def launch(din, dout, nn, batch, t, s):
            assert sm.lib.smfft_synchronize() == 0                              # the prefill of the output, on the null stream
            dc.launch_ptr(din, dout, nn, batch, t, s, stream=stream.value)
            assert hip.hipStreamSynchronize(stream) == 0
        _check_rows(run(sm, dc, x, type, sine, launch=launch), dm.chain(x, type, sine), n, f"stream n={n} {_name(type, sine)}")
    assert hip.hipStreamDestroy(stream) == 0


def test_benchmark_form_adds_to_the_timer(sm, dc):
    """the library's smfft_dct_benchmark adds its milliseconds to a non-zero total and fills the output; so does the mirror's"""
    n = 2048
    x = rh.rand(np.random.default_rng(12), (300, n))
    total = ctypes.c_double(1.0)

    def c_form(din, dout, nn, batch, t, s):
        assert dc.lib().smfft_dct_benchmark(din, dout, nn, batch, t, int(s), ctypes.byref(total)) == 0
        assert total.value > 1.0
    out = run(sm, dc, x, 2, False, launch=c_form)
    _check_rows(out, dm.chain(x, 2, False), n, "benchmark form")

    def mirror(din, dout, nn, batch, t, s):
        status, ms = dc.benchmark(din, dout, nn, batch, t, s)
        assert status == 0 and ms > 0.0
    assert np.array_equal(rh.bits(run(sm, dc, x, 2, False, launch=mirror)), rh.bits(out))


def test_host_round_trip(sm, dc):
    """dct.dct / dct.dst on 1-D, 3-D and float64 host arrays: float32 of the input's shape with the bits of the device-pointer launch;
    an empty batch returns an empty array; unsupported lengths and types raise ValueError"""
    rng = np.random.default_rng(7)
    x1 = rng.standard_normal(1024)                                                  # 1-D float64
    got = dc.dct(x1)
    assert got.shape == (1024,) and got.dtype == np.float32
    assert np.array_equal(rh.bits(got), rh.bits(run(sm, dc, x1.astype(np.float32)[None], 2, False)[0]))
    _check_rows(got[None], dm.chain(x1.astype(np.float32)[None], 2, False), 1024, "dct() 1-D")
    x3 = rh.rand(rng, (2, 3, 512))
    for type in (2, 3):
        got = dc.dst(x3, type=type)
        assert got.shape == x3.shape and got.dtype == np.float32
        assert np.array_equal(rh.bits(got.reshape(6, 512)), rh.bits(run(sm, dc, x3.reshape(6, 512), type, True)))
    back = dc.dct(dc.dct(x3), type=3) / np.float32(2 * 512)
    _check_rows(back.reshape(6, 512), x3.reshape(6, 512).astype(np.float64), 512, "dct(dct(x), 3) / 2n", factor=2.0)
    empty = dc.dct(np.zeros((0, 512), np.float32))
    assert empty.shape == (0, 512) and empty.dtype == np.float32
    for bad in (np.zeros(256), np.zeros(500), np.zeros((2, 16384))):
        with pytest.raises(ValueError):
            dc.dct(bad)
    with pytest.raises(ValueError):
        dc.dst(x3, type=4)
    assert ROW_REL_L2 == 1e-6 and ROW_MAX == 5e-6


def test_tensors_on_the_device(sm, dc):
    """dct.launch / dct.dct / dct.dst on float32 torch tensors on the device: a new tensor, a given one, and x itself (in place) hold
    the bits of the device-pointer launch; a tensor that is not contiguous float32 is refused"""
    import torch
    rng = np.random.default_rng(8)
    x = rh.rand(rng, (5, 3, 2048))
    t = torch.from_numpy(x).cuda()
    for type, sine in TRANSFORMS:
        want = run(sm, dc, x.reshape(15, 2048), type, sine).reshape(x.shape)
        got = (dc.dst if sine else dc.dct)(t, type=type)
        assert got.shape == t.shape and got.dtype == torch.float32 and got.is_cuda and got.data_ptr() != t.data_ptr()
        torch.cuda.synchronize()
        assert np.array_equal(rh.bits(got.cpu().numpy()), rh.bits(want)), (type, sine)
        out = torch.full_like(t, float("nan"))
        assert dc.launch(t, out, type=type, sine=sine) is out
        work = t.clone()
        assert dc.launch(work, work, type=type, sine=sine) is work
        torch.cuda.synchronize()
        assert np.array_equal(rh.bits(out.cpu().numpy()), rh.bits(want)) and np.array_equal(rh.bits(work.cpu().numpy()), rh.bits(want)), (type, sine)
    with pytest.raises(TypeError):
        dc.launch(t.double())
    with pytest.raises(ValueError):
        dc.launch(t[:, :, ::2])
    with pytest.raises(ValueError):
        dc.launch(t, torch.empty(5, 3, 1024, device="cuda"))

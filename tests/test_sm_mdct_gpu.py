"""The DCT-IV / MDCT kernels on an MI355X (smfft_dct4_launch, smfft_mdct_launch, smfft_imdct_launch, smfft_amd.mdct; dct4_kernel,
mdct_kernel and imdct_kernel per inner length M = n / 2 = 256 ... 4096) against the kernels' chain in fp64, built from NumPy alone
(tools/mdct_model.py with float64, which tests/test_sm_mdct_cpu.py holds to the sums of the definition and to scipy): Gaussian rows at
every length for dct4, dst4, mdct (with a window and without) and imdct, as a single row, with a ragged last tile and one row past a
full tile; unit impulses at the ends of a row and at the fold boundaries against the cosine and sine columns of the definition; the
involution and the reconstruction of a signal from its lapped transform; frames read from the signal itself against copied-out rows;
a NaN row among others; the place of a row in its batch, the grid and in place against out of place, none of which may show in the
bits; the grid-stride loop; guarded buffers around input, window and output; 64-bit offsets; a caller's stream, the benchmark forms
and tensors.

Every run through `run` goes into an output prefilled with 0xFF (NaN), with a guard of 4096 elements of 0x5A on both sides that must
stay untouched; the input ends where its allocation ends.  Elements are float32: 4 bytes.

The bound, per row against fp64: ||d||_2 / ||want||_2 <= ROW_REL_L2 = 1e-6 and max |d| / max |want| <= ROW_MAX = 5e-6, the project's
bounds for its fused chains (tests/fir_gpu_harness.py).  An fp32 NumPy model of the chain gave relL2 <= 7e-8 and max <= 1.2e-7
(tests/test_sm_mdct_cpu.py); the kernels measured relL2 <= 2.4e-7 and max <= 5.1e-7 on single launches when this was written.  Round
trips of two launches are held to twice the bounds (measured 2.4e-7 / 4.3e-7).  The tests print the worst figures they
measure per transform."""
import ctypes
import os
import sys

import numpy as np
import pytest

from tests import guarded_region
from tests import rows_gpu_harness as rh
from tests.fir_gpu_harness import GUARD, ROW_MAX, ROW_REL_L2

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import mdct_model as mm  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = [512, 1024, 2048, 4096, 8192]
KINDS = ["dct4", "dst4", "mdct", "mdct_flat", "imdct"]       # mdct_flat: the MDCT with a NULL window
WORST = rh.Worst()      # kind -> [relL2, max / max]: the worst figures measured in this run
E = 4                       # bytes per element


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def md():
    from smfft_amd import mdct
    mdct.lib()              # a missing library raises here: the tests fail, they do not skip
    return mdct


def _ffts(n):
    return 8192 // n


def _window(kind, n):
    """a window that is no symmetry of its own: the sine window times a slow ramp, float32"""
    if kind not in ("mdct", "imdct"):
        return None
    return (mm.sine_window(n) * (1.0 + 0.25 * np.arange(2 * n) / (2 * n))).astype(np.float32)


def _in_out(kind, n):
    """floats per row on the input and on the output side"""
    return (2 * n if kind.startswith("mdct") else n), (2 * n if kind == "imdct" else n)


def _want(kind, x, w):
    if kind in ("dct4", "dst4"):
        return mm.chain(x, kind == "dst4")
    return mm.imdct_chain(x, w) if kind == "imdct" else mm.mdct_chain(x, w)


def _check_rows(got, want, kind, what, factor=1.0):
    """got, want: (batch, n); prints the worst row figures before it asserts"""
    d = got.astype(np.float64) - want
    l2 = np.linalg.norm(d, axis=1) / np.maximum(np.linalg.norm(want, axis=1), 1e-300)
    mx = np.max(np.abs(d), axis=1) / np.maximum(np.max(np.abs(want), axis=1), 1e-300)
    worst = WORST.record(kind, l2, mx)
    print(f"{what}: worst row relL2 = {l2.max():.3e}, max |d| / max |want| = {mx.max():.3e}  ({kind} so far: {worst[0]:.3e}, {worst[1]:.3e})")
    assert l2.max() <= factor * ROW_REL_L2 and mx.max() <= factor * ROW_MAX, \
        f"{what}: row {int(np.argmax(l2))} relL2 = {l2.max():.3e}, row {int(np.argmax(mx))} max = {mx.max():.3e}"


def _launch(md, kind, pin, pout, pw, n, batch, grid=None, stream=0):
    if kind in ("dct4", "dst4"):
        md.dct4_ptr(pin, pout, n, batch, kind == "dst4", stream=stream, grid=grid)
    elif kind == "imdct":
        md.imdct_ptr(pin, pout, pw, n, batch, stream=stream, grid=grid)
    else:
        md.mdct_ptr(pin, pout, pw, n, batch, 1, n, 2 * n, stream=stream, grid=grid)


def run(sm, md, kind, x, w=None, finite=True, launch=None, in_place=False, grid=None):
    """one launch through the device-pointer API on a copy of x = (batch, floats per input row) float32 and of the window w (2 n floats
    or None).  Out of place: the input ends where its allocation ends and the output lies between guards; in place (dct4 / dst4): the
    rows lie between guards.  Returns the (batch, floats per output row) result after checking the guards and (finite) that no NaN of
    the prefill is left.  launch(d_in, d_out, d_window, n, batch): how to launch, when not on the null stream through the mirror"""
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    batch = x.shape[0]
    n = x.shape[1] // 2 if kind.startswith("mdct") else x.shape[1]
    nin, nout = _in_out(kind, n)
    assert x.shape[1] == nin and (w is None or (w.dtype == np.float32 and w.shape == (2 * n,)))
    dout, pout = rh.guarded(sm, batch * nout, E)
    din = dw = None
    try:
        if in_place:
            assert nin == nout and sm.lib.smfft_memcpy_h2d(pout, x.ctypes.data, x.nbytes) == 0
            pin = pout
        else:
            din = sm.DeviceBuffer(x.nbytes)
            assert din.nbytes == x.nbytes and sm.lib.smfft_memcpy_h2d(din.ptr, x.ctypes.data, x.nbytes) == 0
            pin = din.ptr
        if w is not None:
            dw = sm.DeviceBuffer(w.nbytes)
            assert sm.lib.smfft_memcpy_h2d(dw.ptr, w.ctypes.data, w.nbytes) == 0
        pw = None if dw is None else dw.ptr
        if launch is None:
            _launch(md, kind, pin, pout, pw, n, batch, grid)
        else:
            launch(pin, pout, pw, n, batch)
        assert sm.lib.smfft_synchronize() == 0
        return rh.collect(dout, batch * nout, np.float32, finite=finite).reshape(batch, nout)
    finally:
        for buf in (din, dout, dw):
            if buf is not None:
                buf.free()


# ---- 1: fp64 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", LENGTHS)
def test_against_fp64(sm, md, n, kind, which):
    """batch = 1 (a single row), 17 (a ragged last tile at sixteen rows per workgroup, several tiles above) and 8192 / n + 1 (one row
    past a full tile)"""
    batch = (1, 17, _ffts(n) + 1)[which]
    nin, nout = _in_out(kind, n)
    x = rh.rand(np.random.default_rng(10 * n + batch), (batch, nin))
    w = _window(kind, n)
    got = run(sm, md, kind, x, w)
    assert got.shape == (batch, nout) and got.dtype == np.float32
    _check_rows(got, _want(kind, x, w), kind, f"n={n} {kind} batch={batch}")


# ---- 2: exact probes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [512, 8192])
def test_probe_impulses(sm, md, n):
    """unit impulses at j = 0, 1, n-2, n-1 of a row (dct4, dst4, and as coefficients of the imdct) and at 0, 1, the fold boundaries
    N/2, N, 3N/2 and the samples in front of them, 2N-2 and 2N-1 of a frame (mdct): the cosine or sine column of the definition, the
    fp64 formula itself, within the row bounds.  A wrong index in the fold, the unfold or the interleaved store moves or mirrors it"""
    k = np.arange(n)
    js = [0, 1, n // 2, n - 2, n - 1]
    x = np.zeros((len(js), n), np.float32)
    x[np.arange(len(js)), js] = 1
    for kind, f in (("dct4", np.cos), ("dst4", np.sin)):
        want = np.stack([2.0 * f(np.pi * (2 * k + 1) * (2 * j + 1) / (4 * n)) for j in js])
        _check_rows(run(sm, md, kind, x), want, kind, f"n={n} {kind} impulses at {js}")
    w = _window("imdct", n).astype(np.float64)
    j2 = np.arange(2 * n)
    want = np.stack([w * np.cos(np.pi / n * (j2 + 0.5 + n / 2) * (kk + 0.5)) for kk in js])
    _check_rows(run(sm, md, "imdct", x, w.astype(np.float32)), want, "imdct", f"n={n} imdct impulses at {js}")
    js = [0, 1, n // 2 - 1, n // 2, n - 1, n, 3 * n // 2 - 1, 3 * n // 2, 2 * n - 2, 2 * n - 1]
    x = np.zeros((len(js), 2 * n), np.float32)
    x[np.arange(len(js)), js] = 1
    for kind, ww in (("mdct", w), ("mdct_flat", None)):
        want = np.stack([(1.0 if ww is None else ww[j]) * np.cos(np.pi / n * (j + 0.5 + n / 2) * (k + 0.5)) for j in js])
        _check_rows(run(sm, md, kind, x, None if ww is None else ww.astype(np.float32)), want, kind, f"n={n} {kind} impulses at {js}")


@pytest.mark.parametrize("n", LENGTHS)
def test_involution(sm, md, n):
    """dct4(dct4(x)) / (2n) and dst4(dst4(x)) / (2n) return x within twice the row bounds (two launches), batch = 8192 / n + 1"""
    x = rh.rand(np.random.default_rng(20 + n), (_ffts(n) + 1, n))
    for kind in ("dct4", "dst4"):
        back = run(sm, md, kind, run(sm, md, kind, x))
        _check_rows(back.astype(np.float64) / (2 * n), x.astype(np.float64), kind, f"n={n} {kind} twice", factor=2.0)


def _frames(sm, md, flat, w, n, C, F, hop, stride):
    """one MDCT launch over C streams of F frames read from the flat signal itself, which ends with the last frame's last sample where
    its allocation ends; the (C F, n) coefficients from between guards"""
    flat = np.ascontiguousarray(flat)
    assert flat.dtype == np.float32 and flat.shape == ((C - 1) * stride + (F - 1) * hop + 2 * n,)
    dout, pout = rh.guarded(sm, C * F * n, E)
    din, dw = sm.DeviceBuffer(flat.nbytes), sm.DeviceBuffer(w.nbytes)
    try:
        assert din.nbytes == flat.nbytes and sm.lib.smfft_memcpy_h2d(din.ptr, flat.ctypes.data, flat.nbytes) == 0
        assert sm.lib.smfft_memcpy_h2d(dw.ptr, w.ctypes.data, w.nbytes) == 0
        md.mdct_ptr(din.ptr, pout, dw.ptr, n, C, F, hop, stride)
        assert sm.lib.smfft_synchronize() == 0
        return rh.collect(dout, C * F * n, np.float32).reshape(C * F, n)
    finally:
        for buf in (din, dout, dw):
            buf.free()


@pytest.mark.parametrize("n", [512, 8192])
def test_lapped_transform_reconstructs_the_signal(sm, md, n):
    """C = 2 streams of 6 N samples, 5 frames each at hop N in one MDCT launch, one IMDCT launch, the sine window: the overlap-added
    frames over N / 2 are the signal away from its first and last N samples -- time-domain aliasing cancels -- within twice the row
    bounds (two launches) per stretch of N samples.  (The sum is NumPy's here; smfft_amd.mdct.overlap_add is held to it in
    test_tensors_on_the_device.)"""
    C, F = 2, 5
    s = rh.rand(np.random.default_rng(25 + n), (C, (F + 1) * n))
    w = mm.sine_window(n).astype(np.float32)
    X = _frames(sm, md, s.reshape(-1), w, n, C, F, n, (F + 1) * n)
    y = run(sm, md, "imdct", X, w).reshape(C, F, 2 * n)
    got = mm.overlap_add(y.astype(np.float64))[:, n:-n] / (n / 2)
    _check_rows(got.reshape(-1, n), s[:, n:-n].astype(np.float64).reshape(-1, n), "lapped", f"N={n} overlap-add of the IMDCT of the MDCT", factor=2.0)


@pytest.mark.parametrize("n", [512, 2048, 8192])
def test_frames_from_the_signal_are_the_copied_rows(sm, md, n):
    """the frames of C = 2 streams at hop N, read from the signal itself, equal the MDCT of the copied-out rows to the bit; so they
    do at stream_stride = L + 12 > L, and at a hop and a stride that are no multiples of four floats (frames at 4-byte alignment)"""
    rng = np.random.default_rng(27 + n)
    C, F = 2, 5
    L = (F + 1) * n
    w = _window("mdct", n)
    for hop, stride in ((n, L), (n, L + 12), (n - 3, L + 5)):
        flat = rh.rand(rng, ((C - 1) * stride + (F - 1) * hop + 2 * n,))
        rows = np.stack([flat[c * stride + f * hop:c * stride + f * hop + 2 * n] for c in range(C) for f in range(F)])
        if (hop, stride) == (n, L):
            assert np.array_equal(rows, mm.frames(flat.reshape(C, L), n).reshape(C * F, 2 * n))
        base = run(sm, md, "mdct", rows, w)
        _check_rows(base, mm.mdct_chain(rows, w), "mdct", f"N={n} copied-out rows, hop {hop}")
        assert np.array_equal(rh.bits(_frames(sm, md, flat, w, n, C, F, hop, stride)), rh.bits(base)), (n, hop, stride)


# ---- 3: isolation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_probe_rows_are_isolated(sm, md, n):
    """batch = 2 (8192 / n) + 1, one row all NaN between finite rows: that row has no finite output and every other row keeps the bits
    of the clean run"""
    F = _ffts(n)
    batch = 2 * F + 1
    row = F + F // 2
    for kind in ("dct4", "dst4", "mdct", "imdct"):
        x = rh.rand(np.random.default_rng(30 + n), (batch, _in_out(kind, n)[0]))
        w = _window(kind, n)
        clean = run(sm, md, kind, x, w)
        bad = x.copy()
        bad[row] = np.nan
        got = run(sm, md, kind, bad, w, finite=False)
        assert np.isnan(got[row]).all(), (n, kind)
        others = np.arange(batch) != row
        assert np.array_equal(rh.bits(got[others]), rh.bits(clean[others])), (n, kind)


@pytest.mark.parametrize("n", LENGTHS)
def test_position_grid_and_in_place_are_invisible(sm, md, n):
    """batch = 3 (8192 / n) + 1 among other Gaussian rows: one row alone, at row 0, at the last slot of the first tile, in the middle
    and as the ragged last row gives the same bits; the launches on 1 and 3 workgroups give the bits of the default launch; and so
    does dct4 / dst4 with d_out == d_in, between guards"""
    F = _ffts(n)
    batch = 3 * F + 1
    places = sorted({0, F - 1, F + F // 2, batch - 1})
    for kind in KINDS:
        rng = np.random.default_rng(40 + n)
        nin = _in_out(kind, n)[0]
        probe, x, w = rh.rand(rng, (1, nin)), rh.rand(rng, (batch, nin)), _window(kind, n)
        x[places] = probe[0]
        alone = run(sm, md, kind, probe, w)
        _check_rows(alone, _want(kind, probe, w), kind, f"n={n} {kind} alone")
        base = run(sm, md, kind, x, w)
        for r in places:
            assert np.array_equal(rh.bits(base[r]), rh.bits(alone[0])), (n, kind, r)
        for grid in (1, 3):
            assert np.array_equal(rh.bits(run(sm, md, kind, x, w, grid=grid)), rh.bits(base)), (n, kind, grid)
        if kind in ("dct4", "dst4"):
            assert np.array_equal(rh.bits(run(sm, md, kind, x, in_place=True)), rh.bits(base)), (n, kind, "in place")
            assert np.array_equal(rh.bits(run(sm, md, kind, x, in_place=True, grid=1)), rh.bits(base)), (n, kind, "in place, one workgroup")


# ---- 4: the grid-stride loop ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_grid_stride_loop(sm, md, kind):
    """n = 512, batch = 100 on grid = 2: seven tiles of sixteen rows, the last one ragged, three or four per workgroup"""
    n, batch = 512, 100
    x = rh.rand(np.random.default_rng(50), (batch, _in_out(kind, n)[0]))
    w = _window(kind, n)
    got = run(sm, md, kind, x, w, grid=2)
    _check_rows(got, _want(kind, x, w), kind, f"grid-stride n={n} batch={batch} {kind}")
    assert np.array_equal(rh.bits(got), rh.bits(run(sm, md, kind, x, w)))


# ---- 5: bounds ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, batch", [(512, 17), (8192, 1)])
def test_bounds(sm, md, n, batch):
    """input, window and output each inside a poisoned allocation with 128 KiB of guard on both sides (tests/guarded_region.py): the
    input, the window and everything around them are unchanged, nothing around the output floats is written, every output is, and the
    bits are those of the plain run, which passes the fp64 bound.  (A read outside the input or the window would pick up the poison, a
    NaN, and show in the result.)"""
    for kind in KINDS:
        nin, nout = _in_out(kind, n)
        x = rh.rand(np.random.default_rng(60 + n), (batch, nin))
        w = _window(kind, n)
        base = run(sm, md, kind, x, w)
        _check_rows(base, _want(kind, x, w), kind, f"n={n} batch={batch} {kind}")
        rin = guarded_region.Region(sm, x.view(np.uint8).reshape(-1), 0, align=4)
        rout = guarded_region.Region(sm, guarded_region.poison(batch * nout * E), 4, align=4)
        rw = None if w is None else guarded_region.Region(sm, w.view(np.uint8).reshape(-1), 4, align=4)
        try:
            _launch(md, kind, rin.ptr, rout.ptr, None if rw is None else rw.ptr, n, batch)
            assert sm.lib.smfft_synchronize() == 0
            rin.outside_unchanged(whole=True)
            if rw is not None:
                rw.outside_unchanged(whole=True)
            got = rout.outside_unchanged(whole=False).view(np.float32).reshape(batch, nout)
            assert np.array_equal(rh.bits(got), rh.bits(base)), (n, batch, kind)
        finally:
            for r in (rin, rout, rw):
                if r is not None:
                    r.buf.free()


# ---- 6: 64-bit offsets ----------------------------------------------------------------------------------------------------------------
def test_offsets_beyond_two_to_the_31(sm, md):
    """dct4, n = 8192, batch = 2^31 / 8192 + 8 rows, 8 GiB, in place: the rows are memset to zero, with Gaussian rows at the first two,
    at those on both sides of byte 2^31, of byte 2^32 and of element 2^31, and at the last two.  Those rows pass the bound, sampled
    zero rows give zeros, and the guard behind the buffer is intact"""
    n = 8192
    batch = (1 << 31) // n + 8
    assert (batch - 8) * n == 1 << 31
    rows = [0, 1, (1 << 29) // n - 1, (1 << 29) // n, (1 << 30) // n - 1, (1 << 30) // n, (1 << 31) // n - 1, (1 << 31) // n, batch - 2, batch - 1]
    zeros = [2, (1 << 29) // n + 1, (1 << 31) // n - 2, (1 << 31) // n + 1, batch - 3]
    x = rh.rand(np.random.default_rng(70), (len(rows), n))
    want = mm.chain(x)
    buf = sm.DeviceBuffer((batch * n + GUARD) * E)
    try:
        assert sm.lib.smfft_memset(buf.ptr, 0, batch * n * E) == 0
        assert sm.lib.smfft_memset(buf.ptr + batch * n * E, 0x5A, GUARD * E) == 0
        for i, r in enumerate(rows):
            assert sm.lib.smfft_memcpy_h2d(buf.ptr + r * n * E, x[i].ctypes.data, n * E) == 0
        md.dct4_ptr(buf.ptr, buf.ptr, n, batch)
        assert sm.lib.smfft_synchronize() == 0
        guard = np.empty(GUARD, np.uint32)
        assert sm.lib.smfft_memcpy_d2h(guard.ctypes.data, buf.ptr + batch * n * E, guard.nbytes) == 0
        assert np.all(guard == 0x5A5A5A5A), "the kernel wrote past its buffer"
        got = np.empty((len(rows), n), np.float32)
        for i, r in enumerate(rows):
            assert sm.lib.smfft_memcpy_d2h(got[i].ctypes.data, buf.ptr + r * n * E, n * E) == 0
        _check_rows(got, want, "dct4", "2^31 rows dct4")
        row = np.empty(n, np.float32)
        for r in zeros:
            assert sm.lib.smfft_memcpy_d2h(row.ctypes.data, buf.ptr + r * n * E, n * E) == 0
            assert not row.any(), f"zero row {r} is not zero everywhere"
    finally:
        buf.free()


# ---- 7: entry forms ---------------------------------------------------------------------------------------------------------------------
def test_caller_stream(sm, md):
    """launch on a stream from hipStreamCreate, then hipStreamSynchronize"""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value
    rng = np.random.default_rng(11)
    for n, kind in ((1024, "dst4"), (4096, "mdct"), (2048, "imdct")):
        x = rh.rand(rng, (37, _in_out(kind, n)[0]))
        w = _window(kind, n)

        def launch(pin, pout, pw, nn, batch):
            assert sm.lib.smfft_synchronize() == 0                              # the prefill of the output, on the null stream
            _launch(md, kind, pin, pout, pw, nn, batch, stream=stream.value)
            assert hip.hipStreamSynchronize(stream) == 0
        _check_rows(run(sm, md, kind, x, w, launch=launch), _want(kind, x, w), kind, f"stream n={n} {kind}")
    assert hip.hipStreamDestroy(stream) == 0


def test_benchmark_forms_add_to_the_timer(sm, md):
    """the library's three *_benchmark entry points add their milliseconds to a non-zero total and fill the output with the bits of
    the plain launch; so do the mirror's"""
    n = 2048
    rng = np.random.default_rng(12)
    total = ctypes.c_double(1.0)
    for kind in ("dct4", "mdct", "imdct"):
        x = rh.rand(rng, (300, _in_out(kind, n)[0]))
        w = _window(kind, n)
        base = run(sm, md, kind, x, w)
        _check_rows(base, _want(kind, x, w), kind, f"benchmark form {kind}")
        before = total.value

        def c_form(pin, pout, pw, nn, batch):
            if kind == "dct4":
                rc = md.lib().smfft_dct4_benchmark(pin, pout, nn, batch, 0, ctypes.byref(total))
            elif kind == "mdct":
                rc = md.lib().smfft_mdct_benchmark(pin, pout, pw, nn, batch, 1, nn, 2 * nn, ctypes.byref(total))
            else:
                rc = md.lib().smfft_imdct_benchmark(pin, pout, pw, nn, batch, ctypes.byref(total))
            assert rc == 0 and total.value > before

        def mirror(pin, pout, pw, nn, batch):
            if kind == "dct4":
                status, ms = md.dct4_benchmark(pin, pout, nn, batch)
            elif kind == "mdct":
                status, ms = md.mdct_benchmark(pin, pout, pw, nn, batch, 1, nn, 2 * nn)
            else:
                status, ms = md.imdct_benchmark(pin, pout, pw, nn, batch)
            assert status == 0 and ms > 0.0
        for form in (c_form, mirror):
            assert np.array_equal(rh.bits(run(sm, md, kind, x, w, launch=form)), rh.bits(base)), (kind, form.__name__)


_TENSOR_SCRIPT = r"""
import sys
import numpy as np
import torch                                  # first: torch initialises the HIP runtime before the library uses it
torch.cuda.init()
sys.path.insert(0, sys.argv[1])
import smfft_amd as sm
from smfft_amd import mdct as md
sm.FFT_init()
rng = np.random.default_rng(8)
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
def pointers(launch, x, shape):
    # the device-pointer launch of the mirror on buffers of the library's own allocator
    din, dout = sm.DeviceBuffer.from_host(np.ascontiguousarray(x)), sm.DeviceBuffer(int(np.prod(shape)) * 4)
    launch(din.ptr, dout.ptr)
    assert sm.lib.smfft_synchronize() == 0
    out = dout.to_host(np.float32, shape)
    din.free(), dout.free()
    return out
n = 1024
x = rng.standard_normal((5, 3, n)).astype(np.float32)
t = torch.from_numpy(x).cuda()
for sine, f in ((False, md.dct4), (True, md.dst4)):
    want = pointers(lambda i, o: md.dct4_ptr(i, o, n, 15, sine), x, x.shape)
    got = f(t)
    assert got.shape == t.shape and got.dtype == torch.float32 and got.is_cuda and got.data_ptr() != t.data_ptr()
    out = torch.full_like(t, float("nan"))
    assert md.launch(t, out, sine=sine) is out
    work = t.clone()
    assert md.launch(work, work, sine=sine) is work
    torch.cuda.synchronize()
    for name, g in (("new", got), ("out", out), ("in place", work)):
        assert np.array_equal(bits(g.cpu().numpy()), bits(want)), (sine, name)
    host = f(x.astype(np.float64))
    assert host.dtype == np.float32 and host.shape == x.shape and np.array_equal(bits(host), bits(want)), sine
    cpu = f(torch.from_numpy(x))
    assert not cpu.is_cuda and np.array_equal(bits(cpu.numpy()), bits(want)), sine
for N in (512, 8192):
    C, F = 2, 5
    s = rng.standard_normal((C, (F + 1) * N)).astype(np.float32)
    ts = torch.from_numpy(s).cuda()
    w = md.sine_window(N, "cuda")
    assert w.is_cuda and w.dtype == torch.float32 and w.shape == (2 * N,)
    X = md.mdct_frames(ts, w, N)
    assert X.shape == (C, F, N) and X.dtype == torch.float32
    rows = torch.stack([ts[:, f * N:f * N + 2 * N] for f in range(F)], dim=1).contiguous()        # the copied-out rows
    Xr = md.mdct(rows, w)
    y = md.imdct(X, w)
    assert Xr.shape == (C, F, N) and y.shape == (C, F, 2 * N)
    z = md.overlap_add(y)
    flat = md.mdct(rows, None)
    torch.cuda.synchronize()
    assert torch.equal(X.view(torch.int32), Xr.view(torch.int32)), N                                # to the bit
    wn = w.cpu().numpy()
    want = pointers(lambda i, o: md.mdct_ptr(i, o, None, N, C * F, 1, N, 2 * N), rows.cpu().numpy(), (C, F, N))
    assert np.array_equal(bits(flat.cpu().numpy()), bits(want)), N
    dw = sm.DeviceBuffer.from_host(wn)
    want = pointers(lambda i, o: md.imdct_ptr(i, o, dw.ptr, N, C * F), X.cpu().numpy(), (C, F, 2 * N))
    dw.free()
    assert np.array_equal(bits(y.cpu().numpy()), bits(want)), N
    # overlap_add is the sum of the frames at hop N, and gives the signal back away from its ends
    yn = y.cpu().numpy()
    ref = np.zeros((C, (F + 1) * N), np.float32)
    for f in range(F):
        ref[:, f * N:f * N + 2 * N] += yn[:, f]
    assert z.shape == (C, (F + 1) * N) and np.array_equal(z.cpu().numpy(), ref), N
    d = z.cpu().numpy().astype(np.float64)[:, N:-N] / (N / 2) - s[:, N:-N]
    d, r = d.reshape(-1, N), s[:, N:-N].astype(np.float64).reshape(-1, N)
    l2 = (np.linalg.norm(d, axis=1) / np.linalg.norm(r, axis=1)).max()
    mx = (np.abs(d).max(axis=1) / np.abs(r).max(axis=1)).max()
    print(f"N={N}: overlap_add(imdct(mdct_frames(s))) / (N/2) against s: worst stretch relL2 = {l2:.3e}, max = {mx:.3e}")
    assert l2 <= 2 * float(sys.argv[2]) and mx <= 2 * float(sys.argv[3]), (N, l2, mx)
def refused(exc, f, *a, **k):
    try:
        f(*a, **k)
    except exc:
        return
    raise SystemExit(f"{f.__name__} was not refused with {exc.__name__}")
tw = md.sine_window(n, "cuda")
refused(TypeError, md.launch, t.double())
refused(ValueError, md.launch, t[:, :, ::2])
refused(ValueError, md.launch, t, torch.empty(5, 3, 512, device="cuda"))
refused(ValueError, md.mdct, t, tw)                  # a window of 2 n floats for rows of n = 2 (n / 2) samples
refused(ValueError, md.mdct, t, tw[:n].cpu())        # a window on another device
refused(ValueError, md.mdct_frames, t.reshape(15, n)[:, :n - 1].contiguous(), None, 512)
refused(ValueError, md.imdct, t[:, :, :500].contiguous())
print("ok")
"""


def test_tensors_on_the_device(md):
    """smfft_amd.mdct on torch tensors on the device, in a process of its own in which torch initialises the HIP runtime before the
    library uses it (the order of tests/test_large_gpu.py): dct4 / dst4 / launch (a new tensor, a given one, in place) and the host
    round trips hold the bits of the device-pointer launches; mdct_frames at hop N equals mdct on the copied-out rows to the bit, at
    N = 512 and 8192 with 5 frames and C = 2; imdct and mdct without a window hold the pointer launches' bits; overlap_add is the sum
    of the frames, and overlap_add(imdct(mdct_frames(s))) / (N/2) is the interior of s within twice the row bounds; tensors that are
    not contiguous float32, and windows of another length or device, are refused"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _TENSOR_SCRIPT, root, repr(ROW_REL_L2), repr(ROW_MAX)], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("ok"), p.stdout + p.stderr
    assert ROW_REL_L2 == 1e-6 and ROW_MAX == 5e-6

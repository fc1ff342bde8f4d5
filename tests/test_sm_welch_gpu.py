"""The Welch kernels on an MI355X (smfft_welch_launch, smfft_csd_launch, smfft_amd.welch; welch_kernel and csd_kernel per inner length
M = n / 2 = 256 ... 4096) against the sums of the STFT chain in fp64, built from NumPy alone (tools/welch_model.py on tools/stft_model.py
with float64, which tests/test_sm_welch_cpu.py holds to the sums of the definition and to scipy.signal), and against the STFT library
itself to the bit: Gaussian signals at every length, with the periodic Hann window and with a NULL window; the sequential fp32 sum of
what smfft_stft_launch(kind = 1) stores; a signal crossed with itself through one pointer; one reference stream at y_stride = 0; the
place of a group in its batch, its stream offset and the grid, none of which may show in the bits; a NaN sample among finite ones;
guarded buffers around input, window and output; a caller's stream, the benchmark forms and tensors.

Small shape: streams C = 3, groups G = 6, frames per group T = 3 -- 18 (stream, group) slots: one full tile and a partial one at
M = 256, one slot per tile at M = 4096 -- at hop n / 4 + 1 (frame starts at 4-byte alignment only) and a stream stride 13 floats larger
than the streams need.  Every run goes into an output prefilled with 0xFF (NaN), with a guard of 4096 elements of 0x5A on both sides
that must stay untouched; the signal ends where its allocation ends, so a frame behind the last group would be read past it.

The bounds, per output spectrum against fp64: ||d||_2 / ||ref||_2 <= 2 ROW_REL_L2 + (T - 1) 2^-24 and max |d| / max ref <=
2 ROW_MAX + (T - 1) 2^-24 -- the STFT power kind's bound (tests/test_sm_stft_gpu.py: d|X|^2 = 2 |X| d|X|) plus the sequential sum's, one
rounding of a partial sum that is at most the whole per added frame.  ref is the fp64 spectrum itself for the auto spectra and
sqrt(Pxx Pyy) of the same group for the cross spectra: |d(conj X Y)| <= |dX| |Y| + |X| |dY|, and Cauchy-Schwarz over the frames bounds
sum |X| |Y| by that, whatever the coherence of the two streams.  The fp32 NumPy model gives 7.3e-8 / 1.7e-7 (auto) and 6.6e-8 / 1.3e-7
(cross) at T <= 7 and 1.2e-7 / 3.6e-7 and 1.1e-7 / 3.2e-7 at T = 64 (tests/test_sm_welch_cpu.py).  The tests print the worst figures they measure per kind."""
import ctypes
import os
import sys

import numpy as np
import pytest

from tests import guarded_region
from tests import rows_gpu_harness as rh
from tests.fir_gpu_harness import ROW_MAX, ROW_REL_L2

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import stft_model as mm  # noqa: E402
import welch_model as wm  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = [512, 1024, 2048, 4096, 8192]
WORST = rh.Worst()          # kind -> [relL2, max / max]: the worst figures measured in this run
E = 4                       # bytes per float
C, G, T = 3, 6, 3           # streams, groups per stream and frames per group of the small shape
F = G * T


def l2_bound(t):
    return 2 * ROW_REL_L2 + (t - 1) * 2.0 ** -24


def max_bound(t):
    return 2 * ROW_MAX + (t - 1) * 2.0 ** -24


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def wl():
    from smfft_amd import welch
    welch.lib()             # a missing library raises here: the tests fail, they do not skip
    return welch


@pytest.fixture(scope="module")
def st():
    from smfft_amd import stft
    stft.lib()
    return stft


def _hann(n):
    return mm.hann(n).astype(np.float32)


def _ramp(n):
    """a window without zeros or symmetry: Hann times a slow ramp on a pedestal, float32"""
    return (mm.hann(n) * (1.0 + 0.25 * np.arange(n) / n) + 0.25).astype(np.float32)


def _geometry(n, frames=F, streams=C):
    """(hop, stream_stride, floats of the signal): frame starts at 4-byte alignment only, streams 13 floats further apart than they need
    to be, and the signal ends with the last frame's last sample"""
    hop = n // 4 + 1
    stride = (frames - 1) * hop + n + 13
    return hop, stride, (streams - 1) * stride + (frames - 1) * hop + n


def _frames_of(flat, n, streams, frames, hop, stride):
    """the frames of the flat signal, copied out: (streams, frames, n)"""
    return np.stack([np.stack([flat[c * stride + f * hop:c * stride + f * hop + n] for f in range(frames)]) for c in range(streams)])


def _pair(rng, total):
    """x and y = 0.7 (x delayed by 3 samples) + 0.5 noise: a cross spectrum that is neither zero nor trivial"""
    x = rh.rand(rng, (total,))
    y = (0.5 * rng.standard_normal(total)).astype(np.float32)
    y[3:] += np.float32(0.7) * x[:-3]
    return x, y


def _check(got, want, kind, what, t, norm=None):
    """got, want: (spectra, M + 1); prints the worst figures before it asserts"""
    l2, mx = wm.errors(got, want, norm)
    worst = WORST.record(kind, l2, mx)
    print(f"{what}: worst relL2 = {l2.max():.3e}, max |d| / max ref = {mx.max():.3e}  ({kind} so far: {worst[0]:.3e}, {worst[1]:.3e})")
    assert l2.max() <= l2_bound(t) and mx.max() <= max_bound(t), \
        f"{what}: spectrum {int(np.argmax(l2))} relL2 = {l2.max():.3e}, spectrum {int(np.argmax(mx))} max = {mx.max():.3e}"


def run(sm, wl, x, y, w, n, streams, groups, t, hop, x_stride, y_stride=None, grid=None, finite=True, launch=None):
    """one launch through the device-pointer API on copies of the flat float32 signals, which end where their allocations end, and of
    the window w (n floats or None).  y None: the auto spectra of x, (streams * groups, n / 2 + 1) float32; y "same": the cross spectra
    of x with itself through one pointer; y an array: the cross spectra, complex64 -- from between guards, after checking them and
    (finite) that no NaN of the prefill is left.  launch(d_x, d_y, d_out, d_window): how to launch, when not on the null stream through
    the mirror"""
    x = np.ascontiguousarray(x)
    frames = groups * t
    assert x.dtype == np.float32 and x.shape == ((streams - 1) * x_stride + (frames - 1) * hop + n,)
    assert w is None or (w.dtype == np.float32 and w.shape == (n,))
    cross = y is not None
    bins = n // 2 + 1
    floats = streams * groups * bins * (2 if cross else 1)
    dout, pout = rh.guarded(sm, floats, E)
    dx, dw = rh.upload(sm, x), None if w is None else rh.upload(sm, w)
    dy = None
    ys = x_stride if y_stride is None else y_stride
    if cross and not isinstance(y, str):
        y = np.ascontiguousarray(y)
        assert y.dtype == np.float32 and y.shape == ((streams - 1) * ys + (frames - 1) * hop + n,)
        dy = rh.upload(sm, y)
    try:
        pw = None if dw is None else dw.ptr
        py = None if not cross else dx.ptr if dy is None else dy.ptr
        if launch is not None:
            launch(dx.ptr, py, pout, pw)
        elif cross:
            wl.csd_ptr(dx.ptr, py, pout, pw, n, streams, groups, t, hop, x_stride, ys, grid=grid)
        else:
            wl.launch_ptr(dx.ptr, pout, pw, n, streams, groups, t, hop, x_stride, grid=grid)
        assert sm.lib.smfft_synchronize() == 0
        out = rh.collect(dout, floats, np.float32, finite=finite)
        return (out.view(np.complex64) if cross else out).reshape(streams * groups, bins)
    finally:
        for buf in (dx, dy, dout, dw):
            if buf is not None:
                buf.free()


def run_power(sm, st, x, w, n, streams, frames, hop, stride):
    """what smfft_stft_launch(kind = 1) stores for the same frames: (streams, frames, n / 2 + 1) float32"""
    bins = n // 2 + 1
    dout, pout = rh.guarded(sm, streams * frames * bins, E)
    dx, dw = rh.upload(sm, x), None if w is None else rh.upload(sm, w)
    try:
        st.launch_ptr(dx.ptr, pout, None if dw is None else dw.ptr, n, streams, frames, hop, stride, power=True)
        assert sm.lib.smfft_synchronize() == 0
        return rh.collect(dout, streams * frames * bins, np.float32).reshape(streams, frames, bins)
    finally:
        for buf in (dx, dout, dw):
            if buf is not None:
                buf.free()


# ---- 1, 2: fp64 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", ["hann", "null"])
@pytest.mark.parametrize("n", LENGTHS)
def test_auto_against_fp64(sm, wl, n, window):
    """3 streams of 6 groups of 3 frames: every output spectrum inside the bounds of the sum of T = 3 powers"""
    hop, stride, total = _geometry(n)
    x = rh.rand(np.random.default_rng(7 * n + len(window)), (total,))
    w = _hann(n) if window == "hann" else None
    got = run(sm, wl, x, None, w, n, C, G, T, hop, stride)
    assert got.shape == (C * G, n // 2 + 1) and got.dtype == np.float32
    want = wm.auto(_frames_of(x, n, C, F, hop, stride), T, w).reshape(C * G, -1)
    _check(got, want, "auto", f"n={n} auto window={window}", T)


@pytest.mark.parametrize("window", ["hann", "null"])
@pytest.mark.parametrize("n", LENGTHS)
def test_cross_against_fp64(sm, wl, n, window):
    """y = 0.7 (x delayed by 3) + 0.5 noise: the error of every cross spectrum against sqrt(Pxx Pyy) of its group, inside the same
    bounds; the imaginary parts of bins 0 and M are +0"""
    hop, stride, total = _geometry(n)
    x, y = _pair(np.random.default_rng(9 * n + len(window)), total)
    w = _hann(n) if window == "hann" else None
    got = run(sm, wl, x, y, w, n, C, G, T, hop, stride)
    assert got.shape == (C * G, n // 2 + 1) and got.dtype == np.complex64
    fx, fy = _frames_of(x, n, C, F, hop, stride), _frames_of(y, n, C, F, hop, stride)
    want = wm.cross(fx, fy, T, w).reshape(C * G, -1)
    norm = np.sqrt(wm.auto(fx, T, w) * wm.auto(fy, T, w)).reshape(C * G, -1)
    assert np.abs(want).max() > 0.3 * norm.max()                 # the pair is coherent: the cross spectrum is not noise
    _check(got, want, "cross", f"n={n} cross window={window}", T, norm)
    assert not rh.bits(got.imag[:, [0, n // 2]]).any(), "the imaginary parts of bins 0 and M are not +0"


# ---- 3: the STFT library's bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_auto_is_the_sequential_sum_of_the_stft_powers(sm, wl, st, n):
    """the auto spectra are the fp32 sum, in frame order, of what smfft_stft_launch(kind = 1) stores for the same frames, to the bit;
    with T = 1 they are those powers themselves; at n = 512 once more with T = 64 and one group"""
    hop, stride, total = _geometry(n)
    x = rh.rand(np.random.default_rng(20 + n), (total,))
    w = _hann(n)
    p = run_power(sm, st, x, w, n, C, F, hop, stride)
    got = run(sm, wl, x, None, w, n, C, G, T, hop, stride)
    assert np.array_equal(rh.bits(got), rh.bits(wm.sequential_sum(p, T).reshape(C * G, -1))), n
    one = run(sm, wl, x, None, w, n, C, F, 1, hop, stride)
    assert np.array_equal(rh.bits(one), rh.bits(p.reshape(C * F, -1))), n
    if n == 512:
        hop, stride, total = _geometry(n, 64, 1)
        x = rh.rand(np.random.default_rng(21), (total,))
        p = run_power(sm, st, x, None, n, 1, 64, hop, stride)
        got = run(sm, wl, x, None, None, n, 1, 1, 64, hop, stride)
        assert np.array_equal(rh.bits(got), rh.bits(wm.sequential_sum(p, 64).reshape(1, -1)))
        _check(got, wm.auto(_frames_of(x, n, 1, 64, hop, stride), 64).reshape(1, -1), "auto", "n=512 T=64", 64)


# ---- 4: a signal with itself ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_cross_of_a_signal_with_itself(sm, wl, n):
    """the same pointer as both operands: the real part has the auto spectrum's bits and the imaginary part is +0 everywhere"""
    hop, stride, total = _geometry(n)
    x = rh.rand(np.random.default_rng(30 + n), (total,))
    for w in (_ramp(n), None):
        auto = run(sm, wl, x, None, w, n, C, G, T, hop, stride)
        got = run(sm, wl, x, "same", w, n, C, G, T, hop, stride)
        assert np.array_equal(rh.bits(got.real), rh.bits(auto)), n
        assert not rh.bits(got.imag).any(), n


# ---- 5: one reference stream ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_y_stride_zero_is_a_repeated_reference(sm, wl, n):
    """y_stride = 0 gives the bits of the launch on a y buffer that repeats the reference stream C times"""
    hop, stride, total = _geometry(n)
    rng = np.random.default_rng(40 + n)
    x, ref = rh.rand(rng, (total,)), rh.rand(rng, ((F - 1) * hop + n,))
    w = _hann(n)
    y = np.zeros(total, np.float32)
    for c in range(C):
        y[c * stride:c * stride + ref.size] = ref
    base = run(sm, wl, x, y, w, n, C, G, T, hop, stride)
    got = run(sm, wl, x, ref, w, n, C, G, T, hop, stride, y_stride=0)
    assert np.array_equal(rh.bits(got), rh.bits(base)), n


# ---- 6: isolation ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_position_grid_and_batch_are_invisible(sm, wl, n):
    """groups of the small shape -- the first, the last slot of a tile, one in the middle of another stream, the ragged last one -- give
    the same bits launched alone (one stream, one group, at their own offset) as inside the batch; the launches on 1 and 2 workgroups
    (18 slots on 2: the grid-stride loop) give the bits of the default launch.  Both kernels"""
    hop, stride, total = _geometry(n)
    x, y = _pair(np.random.default_rng(50 + n), total)
    w = _ramp(n)
    span = (T - 1) * hop + n
    places = sorted({0, min(8192 // n, C * G) - 1, G + 3, C * G - 1})
    for kind, second in (("auto", None), ("cross", y)):
        base = run(sm, wl, x, second, w, n, C, G, T, hop, stride)
        for r in places:
            at = (r // G) * stride + (r % G) * T * hop
            alone = run(sm, wl, x[at:at + span], None if second is None else second[at:at + span], w, n, 1, 1, T, hop, 1)
            assert np.array_equal(rh.bits(alone[0]), rh.bits(base[r])), (n, kind, r)
        for grid in (1, 2):
            assert np.array_equal(rh.bits(run(sm, wl, x, second, w, n, C, G, T, hop, stride, grid=grid)), rh.bits(base)), (n, kind, grid)


@pytest.mark.parametrize("n", LENGTHS)
def test_nan_stays_in_its_groups(sm, wl, n):
    """one NaN sample in stream 1 makes exactly the groups whose frames contain it NaN -- every bin of them -- and every other group
    keeps the bits of the clean run, for both kernels (the NaN in x)"""
    hop, stride, total = _geometry(n)
    x, y = _pair(np.random.default_rng(60 + n), total)
    w = _ramp(n)
    pos = 2 * T * hop + 5                                # inside frames 3 ... 6 of stream 1: groups 1 and 2
    hit = sorted({G + f // T for f in range(F) if f * hop <= pos < f * hop + n})
    assert hit == [G + 1, G + 2]
    bad = x.copy()
    bad[stride + pos] = np.nan
    others = np.setdiff1d(np.arange(C * G), hit)
    for kind, second in (("auto", None), ("cross", y)):
        clean = run(sm, wl, x, second, w, n, C, G, T, hop, stride)
        got = run(sm, wl, bad, second, w, n, C, G, T, hop, stride, finite=False)
        # (bins 0 and M of a cross spectrum are NaN in their real part; their imaginary part is stored as +0)
        assert np.isnan(got[hit].real).all() and np.isnan(got[hit][:, 1:-1]).all(), (n, kind)
        assert np.array_equal(rh.bits(got[others]), rh.bits(clean[others])), (n, kind)


# ---- 8: bounds -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, groups", [(512, 17), (8192, 2)])
def test_bounds(sm, wl, n, groups):
    """x, y, window and output each inside a poisoned allocation with 128 KiB of guard on both sides (tests/guarded_region.py), the
    float buffers at 4-byte alignment, the signals ending with the last frame of the last group: the inputs and everything around
    them are unchanged, nothing around the output is written, every output element is, and the bits are those of the plain run, which
    passes the fp64 bound.  (A read outside an input -- of a frame behind groups * T, say -- would pick up the poison, a NaN.)"""
    hop, stride, total = _geometry(n, groups * T, 1)
    x, y = _pair(np.random.default_rng(70 + n), total)
    w = _ramp(n)
    fx, fy = _frames_of(x, n, 1, groups * T, hop, stride), _frames_of(y, n, 1, groups * T, hop, stride)
    for kind, second in (("auto", None), ("cross", y)):
        base = run(sm, wl, x, second, w, n, 1, groups, T, hop, stride)
        if second is None:
            _check(base, wm.auto(fx, T, w)[0], kind, f"n={n} groups={groups} auto", T)
        else:
            _check(base, wm.cross(fx, fy, T, w)[0], kind, f"n={n} groups={groups} cross", T, np.sqrt(wm.auto(fx, T, w) * wm.auto(fy, T, w))[0])
        rx = guarded_region.Region(sm, x.view(np.uint8).reshape(-1), 4, align=4)
        ry = guarded_region.Region(sm, y.view(np.uint8).reshape(-1), 12, align=4)
        rout = guarded_region.Region(sm, guarded_region.poison(base.nbytes), 4 if second is None else 8, align=4)
        rw = guarded_region.Region(sm, w.view(np.uint8).reshape(-1), 4, align=4)
        try:
            if second is None:
                wl.launch_ptr(rx.ptr, rout.ptr, rw.ptr, n, 1, groups, T, hop, stride)
            else:
                wl.csd_ptr(rx.ptr, ry.ptr, rout.ptr, rw.ptr, n, 1, groups, T, hop, stride, stride)
            assert sm.lib.smfft_synchronize() == 0
            for r in (rx, ry, rw):
                r.outside_unchanged(whole=True)
            got = rout.outside_unchanged(whole=False).view(np.float32)
            assert np.all(np.isfinite(got)), "outputs left unwritten"
            assert np.array_equal(rh.bits(got), rh.bits(base).reshape(-1)), (n, groups, kind)
        finally:
            for r in (rx, ry, rout, rw):
                r.buf.free()


# ---- 9: entry forms ----------------------------------------------------------------------------------------------------------------------
def test_caller_stream(sm, wl):
    """launch on a stream from hipStreamCreate, then hipStreamSynchronize"""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value
    rng = np.random.default_rng(11)
    for n, cross in ((1024, False), (4096, True)):
        hop, stride, total = _geometry(n)
        x, y = _pair(rng, total)
        w = _hann(n)

        def launch(px, py, pout, pw):
            assert sm.lib.smfft_synchronize() == 0                              # the prefill of the output, on the null stream
            if cross:
                wl.csd_ptr(px, py, pout, pw, n, C, G, T, hop, stride, stride, stream=stream.value)
            else:
                wl.launch_ptr(px, pout, pw, n, C, G, T, hop, stride, stream=stream.value)
            assert hip.hipStreamSynchronize(stream) == 0
        got = run(sm, wl, x, y if cross else None, w, n, C, G, T, hop, stride, launch=launch)
        assert np.array_equal(rh.bits(got), rh.bits(run(sm, wl, x, y if cross else None, w, n, C, G, T, hop, stride))), (n, cross)
    assert hip.hipStreamDestroy(stream) == 0


def test_benchmark_forms_add_to_the_timer(sm, wl):
    """the library's two *_benchmark entry points add their milliseconds to a non-zero total and fill the output with the bits of
    the plain launch; so do the mirror's"""
    n = 2048
    hop, stride, total = _geometry(n)
    x, y = _pair(np.random.default_rng(12), total)
    w = _hann(n)
    timer = ctypes.c_double(1.0)
    for cross in (False, True):
        second = y if cross else None
        base = run(sm, wl, x, second, w, n, C, G, T, hop, stride)
        before = timer.value

        def c_form(px, py, pout, pw):
            if cross:
                rc = wl.lib().smfft_csd_benchmark(px, py, pout, pw, n, C, G, T, hop, stride, stride, ctypes.byref(timer))
            else:
                rc = wl.lib().smfft_welch_benchmark(px, pout, pw, n, C, G, T, hop, stride, ctypes.byref(timer))
            assert rc == 0 and timer.value > before

        def mirror(px, py, pout, pw):
            if cross:
                status, ms = wl.csd_benchmark(px, py, pout, pw, n, C, G, T, hop, stride, stride)
            else:
                status, ms = wl.welch_benchmark(px, pout, pw, n, C, G, T, hop, stride)
            assert status == 0 and ms > 0.0
        for form in (c_form, mirror):
            assert np.array_equal(rh.bits(run(sm, wl, x, second, w, n, C, G, T, hop, stride, launch=form)), rh.bits(base)), (cross, form.__name__)


_TENSOR_SCRIPT = r"""
import os, sys
import numpy as np
import torch                                  # first: torch initialises the HIP runtime before the library uses it
torch.cuda.init()
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tools"))
import smfft_amd as sm
from smfft_amd import welch as wl
import stft_model as mm
import welch_model as wm
sm.FFT_init()
L2, MX = float(sys.argv[2]), float(sys.argv[3])
rng = np.random.default_rng(8)
def check(got, want, norm, t, what):
    l2, mx = wm.errors(got.cpu().numpy(), want, norm)
    print(f"{what}: worst relL2 = {l2.max():.3e}, max = {mx.max():.3e}")
    assert l2.max() <= 2 * L2 + (t - 1) * 2.0 ** -24 and mx.max() <= 2 * MX + (t - 1) * 2.0 ** -24, (what, l2.max(), mx.max())
for n, hop, T, F, window in ((512, 129, 4, 23, "hann"), (2048, 512, 5, 13, "null"), (8192, 2049, 3, 7, "hann")):
    streams, L = 2, (F - 1) * hop + n + 11
    assert F % T                                  # the frames left behind the whole groups go through a second launch
    x = rng.standard_normal((streams, L)).astype(np.float32)
    y = (0.5 * rng.standard_normal((streams, L))).astype(np.float32)
    y[:, 3:] += np.float32(0.7) * x[:, :-3]
    w = wl.hann(n, "cuda") if window == "hann" else None
    w64 = None if w is None else w.cpu().numpy().astype(np.float64)
    dx, dy = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    fx, fy = mm.frames(x, n, hop), mm.frames(y, n, hop)
    assert fx.shape == (streams, F, n)
    pxx, pyy, pxy = wm.auto(fx, F, w64)[:, 0], wm.auto(fy, F, w64)[:, 0], wm.cross(fx, fy, F, w64)[:, 0]
    raw = wl.dynamic_spectrum(dx, n, hop, T, w)
    assert raw.shape == (streams, F // T, n // 2 + 1) and raw.dtype == torch.float32 and raw.is_cuda
    assert wl.groups(L, n, hop, T) == F // T
    check(raw, wm.auto(fx, T, w64), None, T, f"n={n} dynamic_spectrum")
    assert torch.equal(wl.launch(dx, n, hop, T, w).view(torch.int32), raw.view(torch.int32))
    craw = wl.csd_launch(dx, dy, n, hop, T, w)
    assert craw.shape == raw.shape and craw.dtype == torch.complex64
    check(craw, wm.cross(fx, fy, T, w64), np.sqrt(wm.auto(fx, T, w64) * wm.auto(fy, T, w64)), T, f"n={n} csd_launch")
    for scaling in ("density", "spectrum"):
        s = wm.scale(n, F, w64, 3.0, scaling)
        # all F frames: F // T groups of T in one launch, the F % T frames left in a second one, summed in torch
        got = wl.welch(dx, 3.0, w, n, hop, scaling, T)
        assert got.shape == (streams, n // 2 + 1) and got.dtype == torch.float32
        check(got, pxx * s, None, F, f"n={n} welch {scaling}")
        got = wl.csd(dx, dy, 3.0, w, n, hop, scaling, T)
        assert got.dtype == torch.complex64
        check(got, pxy * s, np.sqrt(pxx * pyy) * s, F, f"n={n} csd {scaling}")
    check(wl.welch(dx, 1.0, w, n, hop), pxx * wm.scale(n, F, w64), None, F, f"n={n} welch, default T")
    check(wl.csd(dx, dy[0], 1.0, w, n, hop, T=T)[1:], (wm.cross(fx[1:], fy[:1], F, w64)[:, 0]) * wm.scale(n, F, w64),
          np.sqrt(pxx[1:] * pyy[:1]) * wm.scale(n, F, w64), F, f"n={n} csd against one reference stream")
    coh = wl.coherence(dx, dy, w, n, hop, T).cpu().numpy().astype(np.float64)
    want = wm.coherence(pxx, pyy, pxy)
    keep = pxx * pyy > 1e-6 * (pxx * pyy).max()
    excluded = 1.0 - keep.mean()
    # d(coh) = 2 Re(conj Pxy dPxy) / (Pxx Pyy) - coh (dPxx / Pxx + dPyy / Pyy): each relative error is inside the bound of its spectrum
    # in the max norm times max / value; compare per bin with the three bounds added up
    bound = (2 * MX + (F - 1) * 2.0 ** -24) * (2 * np.sqrt((pxx * pyy).max(axis=1, keepdims=True) / (pxx * pyy))
                                                + pxx.max(axis=1, keepdims=True) / pxx + pyy.max(axis=1, keepdims=True) / pyy)
    worst = (np.abs(coh - want) / bound)[keep].max()
    print(f"n={n} coherence: excluded share {excluded:.3f}, worst |d| / bound = {worst:.3e}, coherence in [{want.min():.3f}, {want.max():.3f}]")
    assert excluded == 0.0 and worst <= 1.0 and want.max() <= 1.0 + 1e-12
def refused(exc, f, *a, **k):
    try:
        f(*a, **k)
    except exc:
        return
    raise SystemExit(f"{f.__name__} was not refused with {exc.__name__}")
t = torch.zeros(2, 4096, device="cuda")
refused(TypeError, wl.welch, t.double())
refused(ValueError, wl.welch, t[:, ::2])
refused(ValueError, wl.welch, t, n=500)
refused(ValueError, wl.welch, t, 1.0, wl.hann(512))                      # a window on another device
refused(ValueError, wl.welch, t, scaling="power")
refused(ValueError, wl.csd, t, torch.zeros(3, 4096, device="cuda"))
refused(ValueError, wl.launch, t, 512, 128, 0)
print("ok")
"""


def test_tensors_on_the_device(wl):
    """smfft_amd.welch on torch tensors on the device, in a process of its own in which torch initialises the HIP runtime before the
    library uses it: dynamic_spectrum / launch / csd_launch against the fp64 model per group; welch() and csd() with both scalings and
    coherence() with F not divisible by T -- all F frames, through the second launch -- against the fp64 model under scipy's scaling
    (tests/test_sm_welch_cpu.py holds that to scipy.signal), inside the bounds of a sum of F frames; one reference stream for all
    streams; the coherence per bin inside the bounds of its three spectra, on every bin (the excluded share is 0); refusals"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _TENSOR_SCRIPT, root, repr(ROW_REL_L2), repr(ROW_MAX)], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("ok"), p.stdout + p.stderr
    assert ROW_REL_L2 == 1e-6 and ROW_MAX == 5e-6

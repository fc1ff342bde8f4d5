"""The band-spectrogram kernels on an MI355X (smfft_bands_launch, smfft_amd.bands; bands_kernel per inner length M = n / 2 =
256 ... 4096) against the band sums of the STFT chain in fp64, built from NumPy alone (tools/bands_model.py on tools/stft_model.py with
float64, which tests/test_sm_bands_cpu.py holds to the dense product of the definition), and against the STFT library itself to the
bit: the identity table at every length, with the periodic Hann window and with a NULL window; HTK mel tables; an awkward table (an
empty band, bands of bin 0 and of bin M alone, a band over all bins, overlapping bands, weights of both signs, the cap on the number of
weights, one band); the place of a frame in its batch and the grid, neither of which may show in the bits; a NaN sample among finite
ones; guarded buffers around input, window, plan and output; a caller's stream, the benchmark form, tensors, two plans on one signal.

Small shape: streams C = 3, frames F = 6 -- 18 frames: one full tile and a partial one at M = 256, one slot per tile at M = 4096 -- at
hop n / 4 + 1 (frame starts at 4-byte alignment only) and a stream stride 13 floats larger than the streams need.  Every run goes into
an output prefilled with 0xFF (NaN), with a guard of 4096 elements of 0x5A on both sides that must stay untouched; the signal ends where
its allocation ends, and so does the plan (smfft_bands_prepare writes it into an allocation of exactly plan_bytes).

The bounds, per frame, with w the float32 weights taken exactly, P the fp64 chain's powers, ref = W P and A = |W| P:
    ||got - ref||_2 / ||A||_2    <= kappa_2 2 ROW_REL_L2 + (Lmax + 1) 2^-24,    kappa_2 = ||W||_2 ||P||_2 / ||A||_2
    max |got - ref| / max A      <= kappa_inf 2 ROW_MAX + (Lmax + 1) 2^-24,     kappa_inf = max_b sum_k |w_bk| max P / max A
-- the STFT power kind's bound (tests/test_sm_stft_gpu.py) pushed through W, plus one rounding per product and per partial sum, valid
for any summation order; Lmax is the longest band.  kappa_2 and kappa_inf are computed in fp64 and printed with the worst measured
figures.  A wrong bin, a wrong weight or an off-by-one at a band edge is an error of 1e-2 or more."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

from tests import guarded_region
from tests import rows_gpu_harness as rh
from tests.fir_gpu_harness import ROW_MAX, ROW_REL_L2

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import bands_model as bm  # noqa: E402
import stft_model as mm  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = [512, 1024, 2048, 4096, 8192]
WORST = rh.Worst()          # kind -> [relL2, max / max]: the worst figures measured in this run
E = 4                       # bytes per float
C, F = 3, 6                 # streams and frames per stream of the small shape
RATE = 16000


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def bd():
    from smfft_amd import bands
    bands.lib()             # a missing library raises here: the tests fail, they do not skip
    return bands


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


@functools.lru_cache(maxsize=None)
def _signal(n, seed):
    """the small shape's signal of seed, and the fp64 chain's powers of its frames under the Hann window, the ramp and no window:
    computed once per length and shared (read only)"""
    hop, stride, total = _geometry(n)
    x = rh.rand(np.random.default_rng(seed), (total,))
    fr = _frames_of(x, n, C, F, hop, stride)
    x.setflags(write=False)
    powers = {name: mm.chain(fr, w, np.float64, power=True).reshape(C * F, -1) for name, w in (("hann", _hann(n)), ("ramp", _ramp(n)), ("null", None))}
    return x, powers


def _window(name, n):
    return {"hann": _hann(n), "ramp": _ramp(n), "null": None}[name]


@functools.lru_cache(maxsize=None)
def _mel(n, n_mels):
    from smfft_amd import bands
    first, count, w = bands.from_dense(n, bands.mel_filterbank(n, RATE, n_mels))
    return first, count, w


def _identity(n):
    bins = n // 2 + 1
    return np.arange(bins, dtype=np.int32), np.ones(bins, np.int32), np.ones(bins, np.float32)


@functools.lru_cache(maxsize=None)
def _awkward(n, cap):
    """T + 3 bands (T = n / 32 threads serve a slot: no multiple of T): an empty band, a band of bin 0 alone, one of bin M alone, one
    over all M + 1 bins, and overlapping bands at random places with standard normal weights; cap: two more bands over all bins and
    the rest sized so that the weights number exactly 4 (M + 1)"""
    M = n // 2
    bins, B = M + 1, n // 32 + 3
    rng = np.random.default_rng(1000 + n + cap)
    first, count = [7, 0, M, 0], [0, 1, 1, bins]
    if cap:
        first, count = first + [0, 0], count + [bins, bins]
        rest = B - len(first)
        share = [(bins - 2) // rest] * rest                      # 4 (M + 1) - 3 (M + 1) - 2 weights are left
        share[-1] += (bins - 2) - sum(share)
        count += share
    else:
        count += [int(c) for c in rng.integers(1, 41, B - len(first))]
    first += [int(rng.integers(0, bins - c + 1)) for c in count[len(first):]]
    first, count = np.array(first, np.int32), np.array(count, np.int32)
    assert first.size == B and B % (n // 32) and (not cap or count.sum() == 4 * bins)
    return first, count, rng.standard_normal(int(count.sum())).astype(np.float32)


def _check(got, P, table, n, kind, what):
    """got: (frames, bands) float32; P: (frames, M + 1) fp64 powers.  Prints kappa and the worst figures before it asserts"""
    W = bm.dense(n, *table)
    ref, A = P @ W.T, P @ np.abs(W).T
    k2, kinf, b2, binf = bm.bounds(W, P, int(np.max(table[1])), ROW_REL_L2, ROW_MAX)
    l2, mx = bm.errors(got, ref, A)
    worst = WORST.record(kind, l2, mx)
    print(f"{what}: kappa_2 = {k2.min():.2f} ... {k2.max():.2f}, kappa_inf = {kinf.min():.2f} ... {kinf.max():.2f}; worst relL2 = {l2.max():.3e} "
          f"(bound {b2.min():.2e}), max |d| / max A = {mx.max():.3e} (bound {binf.min():.2e})  ({kind} so far: {worst[0]:.3e}, {worst[1]:.3e})")
    assert np.all(l2 <= b2) and np.all(mx <= binf), \
        f"{what}: frame {int(np.argmax(l2 / b2))} relL2 = {l2.max():.3e}, frame {int(np.argmax(mx / binf))} max = {mx.max():.3e}"


def run(sm, bd, x, w, n, table, streams, frames, hop, stride, grid=None, finite=True, launch=None):
    """one launch through the device-pointer API on a copy of the flat float32 signal, which ends where its allocation ends, of the
    window w (n floats or None) and of the plan of `table` = (first, count, weights), written by smfft_bands_prepare into an allocation
    of exactly plan_bytes: (streams * frames, bands) float32 from between guards, after checking them and (finite) that no NaN of the
    prefill is left.  launch(d_x, d_out, d_window, d_plan): how to launch, when not on the null stream through the mirror"""
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float32 and x.shape == ((streams - 1) * stride + (frames - 1) * hop + n,)
    assert w is None or (w.dtype == np.float32 and w.shape == (n,))
    bands, nw = len(table[0]), len(table[2])
    floats = streams * frames * bands
    dout, pout = rh.guarded(sm, floats, E)
    dx, dw = rh.upload(sm, x), None if w is None else rh.upload(sm, w)
    dplan = sm.DeviceBuffer(bd.plan_bytes(n, bands, nw))
    try:
        assert bd.prepare_ptr(n, *table, dplan.ptr) == nw
        pw = None if dw is None else dw.ptr
        if launch is not None:
            launch(dx.ptr, pout, pw, dplan.ptr)
        else:
            bd.launch_ptr(dx.ptr, pout, pw, dplan.ptr, n, bands, nw, streams, frames, hop, stride, grid=grid)
        assert sm.lib.smfft_synchronize() == 0
        return rh.collect(dout, floats, np.float32, finite=finite).reshape(streams * frames, bands)
    finally:
        for buf in (dx, dout, dw, dplan):
            if buf is not None:
                buf.free()


def run_power(sm, st, x, w, n, streams, frames, hop, stride):
    """what smfft_stft_launch(kind = 1) stores for the same frames: (streams * frames, n / 2 + 1) float32"""
    bins = n // 2 + 1
    dout, pout = rh.guarded(sm, streams * frames * bins, E)
    dx, dw = rh.upload(sm, x), None if w is None else rh.upload(sm, w)
    try:
        st.launch_ptr(dx.ptr, pout, None if dw is None else dw.ptr, n, streams, frames, hop, stride, power=True)
        assert sm.lib.smfft_synchronize() == 0
        return rh.collect(dout, streams * frames * bins, np.float32).reshape(streams * frames, bins)
    finally:
        for buf in (dx, dout, dw):
            if buf is not None:
                buf.free()


# ---- 1: the STFT library's bits ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", ["hann", "null"])
@pytest.mark.parametrize("n", LENGTHS)
def test_identity_table_is_the_stft_power(sm, bd, st, n, window):
    """bands = M + 1, first[b] = b, count[b] = 1, weight 1.0: what smfft_stft_launch(kind = 1) stores, bit for bit"""
    hop, stride, _ = _geometry(n)
    x, _ = _signal(n, 280 + n)
    w = _window(window, n)
    got = run(sm, bd, x, w, n, _identity(n), C, F, hop, stride)
    assert got.shape == (C * F, n // 2 + 1) and got.dtype == np.float32
    assert np.array_equal(rh.bits(got), rh.bits(run_power(sm, st, x, w, n, C, F, hop, stride))), (n, window)


# ---- 2: mel tables against fp64 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, n_mels", [(n, 40) for n in LENGTHS] + [(8192, 128)])
def test_mel_against_fp64(sm, bd, n, n_mels):
    """HTK mel tables at 16 kHz under the Hann window: every frame's bands inside the bounds"""
    hop, stride, _ = _geometry(n)
    x, powers = _signal(n, 280 + n)
    table = _mel(n, n_mels)
    got = run(sm, bd, x, _hann(n), n, table, C, F, hop, stride)
    assert got.shape == (C * F, n_mels)
    _check(got, powers["hann"], table, n, f"mel{n_mels}", f"n={n} mel {n_mels}")


# ---- 3: an awkward table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [False, True])
@pytest.mark.parametrize("n", [512, 8192])
def test_awkward_table(sm, bd, n, cap):
    """n / 32 + 3 bands: an empty band, whose output is +0 with the sign bit clear; bin 0 alone; bin M alone; all M + 1 bins;
    overlapping bands; weights of both signs; cap: exactly 4 (M + 1) weights.  And a table of one band"""
    hop, stride, _ = _geometry(n)
    x, powers = _signal(n, 280 + n)
    table = _awkward(n, cap)
    assert not cap or len(table[2]) == 4 * (n // 2 + 1)
    got = run(sm, bd, x, _ramp(n), n, table, C, F, hop, stride)
    _check(got, powers["ramp"], table, n, "awkward", f"n={n} awkward cap={cap}")
    assert not rh.bits(got[:, 0]).any(), "the empty band is not +0"
    # the bands of bin 0 and of bin M alone: one product each, inside the power kind's bound on that bin plus the product's rounding
    P = powers["ramp"]
    for band, k in ((1, 0), (2, -1)):
        wb = np.float64(table[2][band - 1])
        assert np.all(np.abs(got[:, band] - wb * P[:, k]) <= abs(wb) * (2 * ROW_MAX * P.max(axis=1) + 2.0 ** -23 * P[:, k])), (n, cap, band)
    if not cap:
        one = (np.array([3], np.int32), np.array([n // 4], np.int32), table[2][:n // 4].copy())
        got = run(sm, bd, x, _ramp(n), n, one, C, F, hop, stride)
        assert got.shape == (C * F, 1)
        _check(got, powers["ramp"], one, n, "awkward", f"n={n} one band")
        nothing = (np.array([0, 5], np.int32), np.zeros(2, np.int32), np.zeros(0, np.float32))
        assert not rh.bits(run(sm, bd, x, None, n, nothing, C, F, hop, stride)).any(), "a table of empty bands does not give +0"


# ---- 4: isolation ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_position_grid_and_batch_are_invisible(sm, bd, n):
    """frames of the small shape -- the first, the last slot of a tile, one in the middle of another stream, the ragged last one -- give
    the same bits launched alone (one stream, one frame, at their own offset) as inside the batch; the launches on 1 and 2 workgroups
    (the grid-stride loop) give the bits of the default launch.  The mel table and the awkward one"""
    hop, stride, _ = _geometry(n)
    x, _ = _signal(n, 280 + n)
    w = _ramp(n)
    places = sorted({0, min(8192 // n, C * F) - 1, F + 3, C * F - 1})
    for name, table in (("mel", _mel(n, 40)), ("awkward", _awkward(n, False))):
        base = run(sm, bd, x, w, n, table, C, F, hop, stride)
        for r in places:
            at = (r // F) * stride + (r % F) * hop
            alone = run(sm, bd, x[at:at + n], w, n, table, 1, 1, hop, 1)
            assert np.array_equal(rh.bits(alone[0]), rh.bits(base[r])), (n, name, r)
        for grid in (1, 2):
            assert np.array_equal(rh.bits(run(sm, bd, x, w, n, table, C, F, hop, stride, grid=grid)), rh.bits(base)), (n, name, grid)


@pytest.mark.parametrize("n", LENGTHS)
def test_nan_stays_in_its_frames(sm, bd, n):
    """one NaN sample in stream 1 makes the bands of exactly the frames that contain it NaN -- every band that has a bin -- and every
    other frame keeps the bits of the clean run"""
    hop, stride, _ = _geometry(n)
    x, _ = _signal(n, 280 + n)
    w = _ramp(n)
    table = _awkward(n, False)
    pos = 2 * hop + 5                                    # inside frames 0 ... 2 of stream 1 (hop > n / 4: frame 3 starts behind it)
    hit = sorted(F + f for f in range(F) if f * hop <= pos < f * hop + n)
    assert hit and len(hit) < F
    bad = x.copy()
    bad[stride + pos] = np.nan
    others = np.setdiff1d(np.arange(C * F), hit)
    clean = run(sm, bd, x, w, n, table, C, F, hop, stride)
    got = run(sm, bd, bad, w, n, table, C, F, hop, stride, finite=False)
    filled = table[1] > 0
    assert np.isnan(got[hit][:, filled]).all() and not rh.bits(got[hit][:, ~filled]).any(), n
    assert np.array_equal(rh.bits(got[others]), rh.bits(clean[others])), n


# ---- 6: bounds -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, frames", [(512, 37), (8192, 3)])
def test_bounds(sm, bd, n, frames):
    """x, window, plan and output each inside a poisoned allocation with 128 KiB of guard on both sides (tests/guarded_region.py), at
    4-byte alignment, the signal ending with the last frame: the inputs and everything around them are unchanged, nothing around the
    output is written, every output element is, and the bits are those of the plain run, which passes the fp64 bound.  (A read outside
    an input -- of a weight behind the plan, say -- would pick up the poison, a NaN.)"""
    hop, stride, total = _geometry(n, frames, 1)
    x = rh.rand(np.random.default_rng(70 + n), (total,))
    w = _ramp(n)
    table = _awkward(n, True)
    base = run(sm, bd, x, w, n, table, 1, frames, hop, stride)
    P = mm.chain(_frames_of(x, n, 1, frames, hop, stride), w, np.float64, power=True)[0]
    _check(base, P, table, n, "awkward", f"n={n} frames={frames} bounds")
    plan = bd.tables(n, *table)
    bands, nw = len(table[0]), len(table[2])
    assert plan.nbytes == 12 * bands + 4 * nw
    rx = guarded_region.Region(sm, x.view(np.uint8).reshape(-1), 4, align=4)
    rp = guarded_region.Region(sm, plan, 12, align=4)
    rout = guarded_region.Region(sm, guarded_region.poison(base.nbytes), 4, align=4)
    rw = guarded_region.Region(sm, w.view(np.uint8).reshape(-1), 4, align=4)
    try:
        bd.launch_ptr(rx.ptr, rout.ptr, rw.ptr, rp.ptr, n, bands, nw, 1, frames, hop, stride)
        assert sm.lib.smfft_synchronize() == 0
        for r in (rx, rp, rw):
            r.outside_unchanged(whole=True)
        got = rout.outside_unchanged(whole=False).view(np.float32)
        assert np.all(np.isfinite(got)), "outputs left unwritten"
        assert np.array_equal(rh.bits(got), rh.bits(base).reshape(-1)), (n, frames)
    finally:
        for r in (rx, rp, rout, rw):
            r.buf.free()


# ---- 7: entry forms ----------------------------------------------------------------------------------------------------------------------
def test_caller_stream(sm, bd):
    """launch on a stream from hipStreamCreate, then hipStreamSynchronize; the plan too is prepared on that stream"""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value
    for n in (1024, 8192):
        hop, stride, _ = _geometry(n)
        x, _ = _signal(n, 280 + n)
        w, table = _hann(n), _mel(n, 40)
        bands, nw = len(table[0]), len(table[2])

        def launch(px, pout, pw, pplan):
            assert sm.lib.smfft_synchronize() == 0                              # the prefill of the output, on the null stream
            assert bd.prepare_ptr(n, *table, pplan, stream=stream.value) == nw
            bd.launch_ptr(px, pout, pw, pplan, n, bands, nw, C, F, hop, stride, stream=stream.value)
            assert hip.hipStreamSynchronize(stream) == 0
        got = run(sm, bd, x, w, n, table, C, F, hop, stride, launch=launch)
        assert np.array_equal(rh.bits(got), rh.bits(run(sm, bd, x, w, n, table, C, F, hop, stride))), n
    assert hip.hipStreamDestroy(stream) == 0


def test_benchmark_form_adds_to_the_timer(sm, bd):
    """smfft_bands_benchmark adds its milliseconds to a non-zero total and fills the output with the bits of the plain launch; so
    does the mirror's"""
    n = 2048
    hop, stride, _ = _geometry(n)
    x, _ = _signal(n, 280 + n)
    w, table = _hann(n), _mel(n, 40)
    bands, nw = len(table[0]), len(table[2])
    timer = ctypes.c_double(1.0)
    base = run(sm, bd, x, w, n, table, C, F, hop, stride)

    def c_form(px, pout, pw, pplan):
        rc = bd.lib().smfft_bands_benchmark(px, pout, pw, pplan, n, bands, nw, C, F, hop, stride, ctypes.byref(timer))
        assert rc == 0 and timer.value > 1.0

    def mirror(px, pout, pw, pplan):
        status, ms = bd.benchmark(px, pout, pw, pplan, n, bands, nw, C, F, hop, stride)
        assert status == 0 and ms > 0.0
    for form in (c_form, mirror):
        assert np.array_equal(rh.bits(run(sm, bd, x, w, n, table, C, F, hop, stride, launch=form)), rh.bits(base)), form.__name__


_TENSOR_SCRIPT = r"""
import os, sys
import numpy as np
import torch                                  # first: torch initialises the HIP runtime before the library uses it
torch.cuda.init()
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tools"))
import smfft_amd as sm
from smfft_amd import bands as bd
import stft_model as mm
import bands_model as bm
sm.FFT_init()
L2, MX = float(sys.argv[2]), float(sys.argv[3])
rng = np.random.default_rng(8)
def check(got, P, table, n, what):
    W = bm.dense(n, *table)
    P = P.reshape(-1, P.shape[-1])
    k2, kinf, b2, binf = bm.bounds(W, P, int(np.max(table[1])), L2, MX)
    l2, mx = bm.errors(got.reshape(-1, got.shape[-1]), P @ W.T, P @ np.abs(W).T)
    print(f"{what}: kappa_2 <= {k2.max():.2f}, kappa_inf <= {kinf.max():.2f}, worst relL2 = {l2.max():.3e}, max = {mx.max():.3e}")
    assert np.all(l2 <= b2) and np.all(mx <= binf), (what, l2.max(), mx.max())
for n, hop, F, window in ((512, 129, 23, "hann"), (2048, 512, 13, "null"), (8192, 2049, 7, "hann")):
    streams, L = 2, (F - 1) * hop + n + 11
    x = rng.standard_normal((streams, L)).astype(np.float32)
    w = bd.hann(n, "cuda") if window == "hann" else None
    w64 = None if w is None else w.cpu().numpy().astype(np.float64)
    dx = torch.from_numpy(x).cuda()
    P = mm.chain(mm.frames(x, n, hop), w64, np.float64, power=True)
    assert P.shape == (streams, F, n // 2 + 1) and bd.frames(L, n, hop) == F
    table = bd.from_dense(n, bd.mel_filterbank(n, 16000, 40, mel_scale="slaney", norm="slaney"))
    plan = bd.prepare(n, *table, device="cuda")
    assert plan.bands == 40 and plan.tensor.dtype == torch.uint8 and plan.tensor.numel() == 12 * 40 + 4 * plan.weights
    got = bd.band_spectrogram(dx, plan, hop, w)
    assert got.shape == (streams, F, 40) and got.dtype == torch.float32 and got.is_cuda
    check(got.cpu().numpy(), P, table, n, f"n={n} band_spectrogram")
    out = torch.full((streams, F, 40), float("nan"), device="cuda")
    assert bd.launch(dx, out, plan, hop, w) is out and torch.equal(out.view(torch.int32), got.view(torch.int32))
    # two plans with different band counts on one signal
    rebin = bd.prepare(n, *bd.uniform_bands(n, 10))
    got10 = bd.band_spectrogram(dx, rebin, hop, w)
    assert got10.shape == (streams, F, -(-(n // 2 + 1) // 10))
    check(got10.cpu().numpy(), P, bd.uniform_bands(n, 10), n, f"n={n} uniform_bands")
    assert torch.equal(bd.band_spectrogram(dx, plan, hop, w).view(torch.int32), got.view(torch.int32))
    # center=True: the frames of the reflect-padded signal
    xp = np.pad(x, ((0, 0), (n // 2, n // 2)), mode="reflect")
    Pc = mm.chain(mm.frames(xp, n, hop), w64, np.float64, power=True)
    htk = bd.from_dense(n, bd.mel_filterbank(n, 16000, 64))
    mel = bd.mel_spectrogram(dx, 16000, n, hop, 64, window=w, center=True)
    assert mel.shape == (streams, Pc.shape[1], 64)
    check(mel.cpu().numpy(), Pc, htk, n, f"n={n} mel_spectrogram center")
    ln = bd.mel_spectrogram(dx, 16000, n, hop, 64, window=w, center=True, log="ln")
    db = bd.mel_spectrogram(dx, 16000, n, hop, 64, window=w, center=True, log="db", floor=1e-3)
    assert torch.allclose(ln, torch.log(mel.clamp(min=1e-10)), rtol=1e-6, atol=1e-6)
    assert torch.allclose(db, 10 * torch.log10(mel.clamp(min=1e-3)), rtol=1e-6, atol=1e-5) and float(db.min()) >= -30.0 - 1e-4
def refused(exc, f, *a, **k):
    try:
        f(*a, **k)
    except exc:
        return
    raise SystemExit(f"{f.__name__} was not refused with {exc.__name__}")
t = torch.zeros(2, 4096, device="cuda")
plan = bd.prepare(512, *bd.uniform_bands(512, 4))
refused(TypeError, bd.band_spectrogram, t.double(), plan, 128)
refused(ValueError, bd.band_spectrogram, t[:, ::2], plan, 128)
refused(ValueError, bd.band_spectrogram, t, plan, 0)
refused(ValueError, bd.band_spectrogram, t, plan, 128, bd.hann(512))               # a window on another device
refused(ValueError, bd.band_spectrogram, t, bd.prepare(512, *bd.uniform_bands(512, 4), device="cpu"), 128)
refused(ValueError, bd.launch, t, torch.zeros(2, 3, 3, device="cuda"), plan, 128)
refused(ValueError, bd.mel_spectrogram, t, 16000, 512, 128, 40, log="log2")
print("ok")
"""


def test_tensors_on_the_device(bd):
    """smfft_amd.bands on torch tensors on the device, in a process of its own in which torch initialises the HIP runtime before the
    library uses it: band_spectrogram / launch with a Slaney mel plan and a re-binning plan on one signal -- two plans with different
    band counts -- and mel_spectrogram with center=True against the fp64 model inside the bounds; the log options against torch on
    the linear output; refusals"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _TENSOR_SCRIPT, root, repr(ROW_REL_L2), repr(ROW_MAX)], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("ok"), p.stdout + p.stderr
    assert ROW_REL_L2 == 1e-6 and ROW_MAX == 5e-6


# ---- 8: two plans ------------------------------------------------------------------------------------------------------------------------
def test_two_plans_on_one_signal(sm, bd):
    """plans of 40 and of 128 bands, alive at once, on one signal at n = 8192, launched in turn: each output is its own table's, to
    the bits of the run that had the signal to itself"""
    n = 8192
    hop, stride, _ = _geometry(n)
    x, powers = _signal(n, 280 + n)
    w = _hann(n)
    tables = (_mel(n, 40), _mel(n, 128))
    alone = [run(sm, bd, x, w, n, t, C, F, hop, stride) for t in tables]
    dx, dw = rh.upload(sm, x), rh.upload(sm, w)
    plans = [sm.DeviceBuffer(bd.plan_bytes(n, len(t[0]), len(t[2]))) for t in tables]
    outs = [rh.guarded(sm, C * F * len(t[0]), E) for t in tables]
    try:
        for t, p in zip(tables, plans):
            bd.prepare_ptr(n, *t, p.ptr)
        for _ in range(2):
            for t, p, (_, pout) in zip(tables, plans, outs):
                bd.launch_ptr(dx.ptr, pout, dw.ptr, p.ptr, n, len(t[0]), len(t[2]), C, F, hop, stride)
        assert sm.lib.smfft_synchronize() == 0
        for t, (dout, _), want in zip(tables, outs, alone):
            got = rh.collect(dout, C * F * len(t[0]), np.float32).reshape(C * F, -1)
            assert np.array_equal(rh.bits(got), rh.bits(want)), len(t[0])
            _check(got, powers["hann"], t, n, f"mel{len(t[0])}", f"n={n} two plans, {len(t[0])} bands")
    finally:
        for buf in [dx, dw] + plans + [o[0] for o in outs]:
            buf.free()

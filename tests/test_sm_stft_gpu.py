"""The STFT kernels on an MI355X (smfft_stft_launch, smfft_istft_launch, smfft_amd.stft; stft_kernel for the complex spectrum and for the
power and istft_kernel per inner length M = n / 2 = 256 ... 4096) against the kernels' chain in fp64, built from NumPy alone
(tools/stft_model.py with float64, which tests/test_sm_stft_cpu.py holds to the sums of the definition, to np.fft.rfft / irfft and to
torch.stft / torch.istft): Gaussian signals at every length, with the periodic Hann window and with a NULL window, in frames that
overlap at a hop that leaves their starts at 4-byte alignment; frames read from the signal itself against copied-out rows; unit
impulses and single bins against the columns of the definition; a NaN sample among finite ones; the place of a frame in its batch, its
stream offset and the grid, none of which may show in the bits; the grid-stride loop; the power against the square of the complex
kind; the round trip; guarded buffers around input, window and output; a caller's stream, the benchmark forms and tensors.

Small shapes: streams = 3 and frames = 7, so M = 256 gets one full tile of 16 frames and a partial one, and M = 4096 one frame per tile.

Every run through `run_stft` / `run_istft` goes into an output prefilled with 0xFF (NaN), with a guard of 4096 elements of 0x5A on
both sides that must stay untouched; the signal ends where its allocation ends.

The bound, per frame against fp64: ||d||_2 / ||want||_2 <= ROW_REL_L2 = 1e-6 and max |d| / max |want| <= ROW_MAX = 5e-6, the project's
bounds for its fused chains (tests/fir_gpu_harness.py), for the complex kind and the inverse; twice those for the power
(d|X|^2 = 2 |X| d|X|) and for the round trip of two launches.  An fp32 NumPy model of the chain gave relL2 <= 7e-8 / max <= 1.1e-7
(complex, inverse) and 1e-7 / 1.7e-7 (power) (tests/test_sm_stft_cpu.py); the kernels measured relL2 <= 1.8e-7 and max <= 4.9e-7
(complex), 1.6e-7 / 3.2e-7 (inverse), 3.2e-7 / 9.6e-7 (power) and 1.8e-7 / 2.4e-7 on the round trip when this was written.  The
tests print the worst figures they measure per kind."""
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

pytestmark = pytest.mark.gpu

LENGTHS = [512, 1024, 2048, 4096, 8192]
KINDS = ["complex", "power", "inverse"]
FACTOR = {"complex": 1.0, "power": 2.0, "inverse": 1.0}
WORST = rh.Worst()      # kind -> [relL2, max / max]: the worst figures measured in this run
E = 4                       # bytes per float
C, F = 3, 7                 # streams and frames per stream of the small shapes


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def st():
    from smfft_amd import stft
    stft.lib()              # a missing library raises here: the tests fail, they do not skip
    return stft


def _spectra(rng, shape):
    """rows of bins, with an imaginary part on bins 0 and M as well: the inverse ignores it"""
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def _hann(n):
    return mm.hann(n).astype(np.float32)


def _ramp(n):
    """a window without zeros or symmetry: Hann times a slow ramp on a pedestal, float32"""
    return (mm.hann(n) * (1.0 + 0.25 * np.arange(n) / n) + 0.25).astype(np.float32)


def _geometry(n):
    """(hop, stream_stride, floats of the signal) of the small shapes: frame starts at 4-byte alignment only, streams further apart
    than they need to be"""
    hop = n // 4 + 1
    stride = (F - 1) * hop + n + 13
    return hop, stride, (C - 1) * stride + (F - 1) * hop + n


def _rows_of(flat, n, streams, frames, hop, stride):
    """the frames of the flat signal, copied out: (streams * frames, n)"""
    return np.stack([flat[c * stride + f * hop:c * stride + f * hop + n] for c in range(streams) for f in range(frames)])


def _want(kind, x, w):
    """the fp64 chain of the copied-out frames (or of rows of bins, for the inverse)"""
    if kind == "inverse":
        return mm.inverse_chain(x, w)
    return mm.chain(x, w, power=kind == "power")


def _check_rows(got, want, kind, what, factor=None):
    """got, want: (rows, .); prints the worst row figures before it asserts"""
    factor = FACTOR[kind] if factor is None else factor
    d = got.astype(want.dtype) - want
    l2 = np.linalg.norm(d, axis=1) / np.maximum(np.linalg.norm(want, axis=1), 1e-300)
    mx = np.max(np.abs(d), axis=1) / np.maximum(np.max(np.abs(want), axis=1), 1e-300)
    worst = WORST.record(kind, l2, mx)
    print(f"{what}: worst row relL2 = {l2.max():.3e}, max |d| / max |want| = {mx.max():.3e}  ({kind} so far: {worst[0]:.3e}, {worst[1]:.3e})")
    assert l2.max() <= factor * ROW_REL_L2 and mx.max() <= factor * ROW_MAX, \
        f"{what}: row {int(np.argmax(l2))} relL2 = {l2.max():.3e}, row {int(np.argmax(mx))} max = {mx.max():.3e}"


def run_stft(sm, st, flat, w, n, streams, frames, hop, stride, kind, grid=None, finite=True, launch=None):
    """one forward launch through the device-pointer API on a copy of the flat float32 signal, which ends with the last frame's last
    sample where its allocation ends, and of the window w (n floats or None).  Returns the (streams * frames, n / 2 + 1) complex64
    ("complex") or float32 ("power") result from between guards, after checking them and (finite) that no NaN of the prefill is left.
    launch(d_in, d_out, d_window): how to launch, when not on the null stream through the mirror"""
    flat = np.ascontiguousarray(flat)
    assert flat.dtype == np.float32 and flat.shape == ((streams - 1) * stride + (frames - 1) * hop + n,)
    assert w is None or (w.dtype == np.float32 and w.shape == (n,))
    bins = n // 2 + 1
    floats = streams * frames * bins * (2 if kind == "complex" else 1)
    dout, pout = rh.guarded(sm, floats, E)
    din, dw = rh.upload(sm, flat), None if w is None else rh.upload(sm, w)
    try:
        pw = None if dw is None else dw.ptr
        if launch is None:
            st.launch_ptr(din.ptr, pout, pw, n, streams, frames, hop, stride, power=kind == "power", grid=grid)
        else:
            launch(din.ptr, pout, pw)
        assert sm.lib.smfft_synchronize() == 0
        out = rh.collect(dout, floats, np.float32, finite=finite)
        return (out.view(np.complex64) if kind == "complex" else out).reshape(streams * frames, bins)
    finally:
        for buf in (din, dout, dw):
            if buf is not None:
                buf.free()


def run_istft(sm, st, X, w, n, grid=None, finite=True, launch=None):
    """one inverse launch on a copy of X = (batch, n / 2 + 1) complex64 and of the window; the (batch, n) float32 result"""
    X = np.ascontiguousarray(X)
    assert X.dtype == np.complex64 and X.ndim == 2 and X.shape[1] == n // 2 + 1
    batch = X.shape[0]
    dout, pout = rh.guarded(sm, batch * n, E)
    din, dw = rh.upload(sm, X), None if w is None else rh.upload(sm, w)
    try:
        pw = None if dw is None else dw.ptr
        if launch is None:
            st.istft_ptr(din.ptr, pout, pw, n, batch, grid=grid)
        else:
            launch(din.ptr, pout, pw)
        assert sm.lib.smfft_synchronize() == 0
        return rh.collect(dout, batch * n, np.float32, finite=finite).reshape(batch, n)
    finally:
        for buf in (din, dout, dw):
            if buf is not None:
                buf.free()


def _case(rng, kind, n):
    """the small shape of a kind: (input, run(input, w, **kw) -> rows, rows of the fp64 chain's input)"""
    if kind == "inverse":
        X = _spectra(rng, (C * F, n // 2 + 1))
        return X, X
    hop, stride, total = _geometry(n)
    flat = rh.rand(rng, (total,))
    return flat, _rows_of(flat, n, C, F, hop, stride)


def _run(sm, st, kind, n, data, w, **kw):
    if kind == "inverse":
        return run_istft(sm, st, data, w, n, **kw)
    hop, stride, _ = _geometry(n)
    return run_stft(sm, st, data, w, n, C, F, hop, stride, kind, **kw)


# ---- 1: fp64 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", ["hann", "null"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", LENGTHS)
def test_against_fp64(sm, st, n, kind, window):
    """3 streams of 7 frames at hop n / 4 + 1 (frame starts at 4-byte alignment only) and a stream stride larger than the streams
    need; 21 rows of bins for the inverse.  Per frame inside the bounds"""
    data, rows = _case(np.random.default_rng(10 * n + len(kind)), kind, n)
    w = _hann(n) if window == "hann" else None
    got = _run(sm, st, kind, n, data, w)
    assert got.shape == (C * F, n if kind == "inverse" else n // 2 + 1)
    assert got.dtype == (np.complex64 if kind == "complex" else np.float32)
    _check_rows(got, _want(kind, rows, w), kind, f"n={n} {kind} window={window}")


# ---- 2: frames from the signal ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [512, 2048, 8192])
def test_frames_from_the_signal_are_the_copied_rows(sm, st, n):
    """the frames of 3 streams read from the signal itself at a hop -- n / 4, n / 4 + 1, an odd 37 and n -- equal the transforms of the
    same frames copied to contiguous rows (hop = stream_stride = n, frames = 1), to the bit, for both kinds"""
    rng = np.random.default_rng(27 + n)
    w = _ramp(n)
    for hop, pad in ((n // 4, 0), (n // 4 + 1, 13), (37, 5), (n, 12)):
        stride = (F - 1) * hop + n + pad
        flat = rh.rand(rng, ((C - 1) * stride + (F - 1) * hop + n,))
        rows = _rows_of(flat, n, C, F, hop, stride)
        for kind in ("complex", "power"):
            base = run_stft(sm, st, rows.reshape(-1), w, n, C * F, 1, n, n, kind)
            _check_rows(base, _want(kind, rows, w), kind, f"n={n} {kind} copied-out rows, hop {hop}")
            got = run_stft(sm, st, flat, w, n, C, F, hop, stride, kind)
            assert np.array_equal(rh.bits(got), rh.bits(base)), (n, hop, stride, kind)


# ---- 3: exact probes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [512, 8192])
def test_probe_impulses(sm, st, n):
    """a unit sample at j = 0, 1, n / 2, n - 1 of a frame gives X[k] = w[j] W_n^{jk} (and its squared modulus w[j]^2) within the
    bounds, with the imaginary parts of X[0] and X[M] exactly +0; a single bin at k = 0, 1, M - 1, M gives its cosine under the
    window, and an imaginary part put on bins 0 and M changes no bit.  A wrong index in the split, the merge or the stores moves or
    mirrors these"""
    M = n // 2
    k = np.arange(M + 1)
    js = [0, 1, n // 2, n - 1]
    x = np.zeros((len(js), n), np.float32)
    x[np.arange(len(js)), js] = 1
    for name, w in (("ramp", _ramp(n)), ("null", None)):
        wj = np.ones(n) if w is None else w.astype(np.float64)
        want = np.stack([wj[j] * np.exp(-2j * np.pi * j * k / n) for j in js])
        got = run_stft(sm, st, x.reshape(-1), w, n, len(js), 1, n, n, "complex")
        _check_rows(got, want, "complex", f"n={n} impulses at {js}, window {name}")
        assert not rh.bits(got.imag[:, [0, M]]).any(), "the imaginary parts of X[0] and X[M] are not +0"
        got = run_stft(sm, st, x.reshape(-1), w, n, len(js), 1, n, n, "power")
        _check_rows(got, np.abs(want) ** 2, "power", f"n={n} power of impulses at {js}, window {name}")
        ks = [0, 1, M - 1, M]
        X = np.zeros((len(ks), M + 1), np.complex64)
        X[np.arange(len(ks)), ks] = 1
        j = np.arange(n)
        want = np.stack([wj * (1.0 if kk in (0, M) else 2.0) * np.cos(2 * np.pi * j * kk / n) / n for kk in ks])
        got = run_istft(sm, st, X, w, n)
        _check_rows(got, want, "inverse", f"n={n} single bins at {ks}, window {name}")
        X[0, 0] = 1 + 3j
        X[3, M] = 1 - 2j
        assert np.array_equal(rh.bits(run_istft(sm, st, X, w, n)), rh.bits(got)), "an imaginary part on bin 0 or M shows"
    # Gaussian frames: the two real bins carry +0 as well
    got = run_stft(sm, st, rh.rand(np.random.default_rng(n), (5 * n,)), _hann(n), n, 5, 1, n, n, "complex")
    assert not rh.bits(got.imag[:, [0, M]]).any()


# ---- 4: isolation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_probe_rows_are_isolated(sm, st, n):
    """one NaN sample in stream 1 makes exactly the frames that cover it NaN -- every bin of them -- and every other frame keeps the
    bits of the clean run, for both kinds; one NaN bin makes its row of the inverse NaN and no other"""
    hop, stride, total = _geometry(n)
    w = _hann(n)
    flat = rh.rand(np.random.default_rng(30 + n), (total,))
    pos = 2 * hop + 5                                  # inside frames 0, 1, 2 of stream 1 (and, with n = 4 hop - 4, of frame 3 not)
    covering = [F + f for f in range(F) if f * hop <= pos < f * hop + n]
    assert covering == [F, F + 1, F + 2]
    bad = flat.copy()
    bad[stride + pos] = np.nan
    others = np.setdiff1d(np.arange(C * F), covering)
    for kind in ("complex", "power"):
        clean = run_stft(sm, st, flat, w, n, C, F, hop, stride, kind)
        got = run_stft(sm, st, bad, w, n, C, F, hop, stride, kind, finite=False)
        assert np.isnan(got[covering]).all(), (n, kind)
        assert np.array_equal(rh.bits(got[others]), rh.bits(clean[others])), (n, kind)
    X = _spectra(np.random.default_rng(31 + n), (C * F, n // 2 + 1))
    clean = run_istft(sm, st, X, w, n)
    X[9, n // 4] = np.nan
    got = run_istft(sm, st, X, w, n, finite=False)
    # (the window's first sample is zero times NaN: NaN as well)
    assert np.isnan(got[9]).all() and np.array_equal(rh.bits(np.delete(got, 9, 0)), rh.bits(np.delete(clean, 9, 0))), n


@pytest.mark.parametrize("n", LENGTHS)
def test_position_and_grid_are_invisible(sm, st, n):
    """frames of the small shape -- the first, the last slot of a tile, one in the middle at another stream offset, the ragged last
    one -- give the same bits alone (one stream, one frame) as inside the batch; the launches on 1 and 3 workgroups give the bits of
    the default launch"""
    places = sorted({0, min(8192 // n, C * F) - 1, F + 3, C * F - 1})
    for kind in KINDS:
        data, rows = _case(np.random.default_rng(40 + n), kind, n)
        w = _ramp(n)
        base = _run(sm, st, kind, n, data, w)
        _check_rows(base, _want(kind, rows, w), kind, f"n={n} {kind} batch")
        for r in places:
            if kind == "inverse":
                alone = run_istft(sm, st, rows[r:r + 1], w, n)
            else:
                alone = run_stft(sm, st, rows[r], w, n, 1, 1, 1, 1, kind)
            assert np.array_equal(rh.bits(alone[0]), rh.bits(base[r])), (n, kind, r)
        for grid in (1, 3):
            assert np.array_equal(rh.bits(_run(sm, st, kind, n, data, w, grid=grid)), rh.bits(base)), (n, kind, grid)


# ---- 5: the grid-stride loop ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_grid_stride_loop(sm, st, kind):
    """n = 512, 40 frames on grid = 2: three tiles of sixteen frames, the last one ragged, one or two per workgroup"""
    n, frames = 512, 40
    rng = np.random.default_rng(50)
    w = _hann(n)
    if kind == "inverse":
        X = _spectra(rng, (frames, n // 2 + 1))
        got, base, want = run_istft(sm, st, X, w, n, grid=2), run_istft(sm, st, X, w, n), _want(kind, X, w)
    else:
        hop = n // 4 + 1
        flat = rh.rand(rng, ((frames - 1) * hop + n,))
        got = run_stft(sm, st, flat, w, n, 1, frames, hop, flat.size, kind, grid=2)
        base = run_stft(sm, st, flat, w, n, 1, frames, hop, flat.size, kind)
        want = _want(kind, _rows_of(flat, n, 1, frames, hop, flat.size), w)
    _check_rows(got, want, kind, f"grid-stride n={n} frames={frames} {kind}")
    assert np.array_equal(rh.bits(got), rh.bits(base))


# ---- 6: the power ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_power_is_the_square_of_the_complex_kind(sm, st, n):
    """kind 1 is re * re + im * im of kind 0's values: within 2 ulp of that sum computed in fp32 from the kind-0 output (one ulp for
    the fused multiply-add of the kernel against the two roundings here, one to spare)"""
    hop, stride, total = _geometry(n)
    flat = rh.rand(np.random.default_rng(55 + n), (total,))
    w = _hann(n)
    X = run_stft(sm, st, flat, w, n, C, F, hop, stride, "complex")
    P = run_stft(sm, st, flat, w, n, C, F, hop, stride, "power")
    ref = X.real * X.real + X.imag * X.imag
    assert ref.dtype == np.float32
    ulps = np.abs(P.astype(np.float64) - ref) / np.spacing(np.maximum(ref, np.float32(1e-30)))
    print(f"n={n}: power against re*re + im*im of the complex kind: at most {ulps.max():.2f} ulp")
    assert ulps.max() <= 2.0, (n, float(ulps.max()))


# ---- 7: the round trip ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [512, 8192])
def test_round_trip(sm, st, n):
    """2 streams, 12 frames at hop n / 4 under the periodic Hann window, one forward and one inverse launch: the overlap-added frames
    over the summed squared window (1.5 there) are the signal on samples [n, end - n) within twice the row bounds (two launches).
    (The sum is NumPy's here; smfft_amd.stft.overlap_add / istft are held to torch in test_tensors_on_the_device.)"""
    streams, frames, hop = 2, 12, n // 4
    L = (frames - 1) * hop + n
    s = rh.rand(np.random.default_rng(25 + n), (streams, L))
    w = _hann(n)
    X = run_stft(sm, st, s.reshape(-1), w, n, streams, frames, hop, L, "complex")
    y = run_istft(sm, st, X, w, n).reshape(streams, frames, n)
    env = mm.overlap_add(np.broadcast_to(w.astype(np.float64) ** 2, (frames, n)), hop)
    assert np.max(np.abs(env[n:-n] - 1.5)) <= 1e-6
    got = mm.overlap_add(y.astype(np.float64), hop)[:, n:-n] / env[n:-n]
    _check_rows(got, s[:, n:-n].astype(np.float64), "round trip", f"n={n} overlap-add of the inverse of the forward frames", factor=2.0)


# ---- 8: bounds ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, frames", [(512, 17), (8192, 1)])
def test_bounds(sm, st, n, frames):
    """input, window and output each inside a poisoned allocation with 128 KiB of guard on both sides (tests/guarded_region.py), the
    float buffers at 4-byte alignment: the input, the window and everything around them are unchanged, nothing around the output is
    written, every output element is, and the bits are those of the plain run, which passes the fp64 bound.  (A read outside the
    input or the window would pick up the poison, a NaN, and show in the result.)"""
    hop = n // 4 + 1
    w = _ramp(n)
    rng = np.random.default_rng(60 + n)
    for kind in KINDS:
        if kind == "inverse":
            x = _spectra(rng, (frames, n // 2 + 1))
            base = run_istft(sm, st, x, w, n)
            rows, out_bytes, in_off = x, frames * n * E, 0
        else:
            x = rh.rand(rng, ((frames - 1) * hop + n,))
            base = run_stft(sm, st, x, w, n, 1, frames, hop, x.size, kind)
            rows, out_bytes, in_off = _rows_of(x, n, 1, frames, hop, x.size), base.nbytes, 4
        _check_rows(base, _want(kind, rows, w), kind, f"n={n} frames={frames} {kind}")
        rin = guarded_region.Region(sm, x.view(np.uint8).reshape(-1), in_off, align=4 if in_off else 8)
        rout = guarded_region.Region(sm, guarded_region.poison(out_bytes), 8 if kind == "complex" else 4, align=4)
        rw = guarded_region.Region(sm, w.view(np.uint8).reshape(-1), 4, align=4)
        try:
            if kind == "inverse":
                st.istft_ptr(rin.ptr, rout.ptr, rw.ptr, n, frames)
            else:
                st.launch_ptr(rin.ptr, rout.ptr, rw.ptr, n, 1, frames, hop, x.size, power=kind == "power")
            assert sm.lib.smfft_synchronize() == 0
            rin.outside_unchanged(whole=True)
            rw.outside_unchanged(whole=True)
            got = rout.outside_unchanged(whole=False).view(np.float32)
            assert np.all(np.isfinite(got)), "outputs left unwritten"
            assert np.array_equal(rh.bits(got), rh.bits(base).reshape(-1)), (n, frames, kind)
        finally:
            for r in (rin, rout, rw):
                r.buf.free()


# ---- 9: entry forms ---------------------------------------------------------------------------------------------------------------------
def test_caller_stream(sm, st):
    """launch on a stream from hipStreamCreate, then hipStreamSynchronize"""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value
    rng = np.random.default_rng(11)
    for n, kind in ((1024, "complex"), (4096, "power"), (2048, "inverse")):
        data, rows = _case(rng, kind, n)
        w = _hann(n)
        hop, stride, _ = _geometry(n)

        def launch(pin, pout, pw):
            assert sm.lib.smfft_synchronize() == 0                              # the prefill of the output, on the null stream
            if kind == "inverse":
                st.istft_ptr(pin, pout, pw, n, C * F, stream=stream.value)
            else:
                st.launch_ptr(pin, pout, pw, n, C, F, hop, stride, power=kind == "power", stream=stream.value)
            assert hip.hipStreamSynchronize(stream) == 0
        _check_rows(_run(sm, st, kind, n, data, w, launch=launch), _want(kind, rows, w), kind, f"stream n={n} {kind}")
    assert hip.hipStreamDestroy(stream) == 0


def test_benchmark_forms_add_to_the_timer(sm, st):
    """the library's two *_benchmark entry points add their milliseconds to a non-zero total and fill the output with the bits of
    the plain launch; so do the mirror's"""
    n = 2048
    rng = np.random.default_rng(12)
    total = ctypes.c_double(1.0)
    hop, stride, _ = _geometry(n)
    for kind in KINDS:
        data, rows = _case(rng, kind, n)
        w = _hann(n)
        base = _run(sm, st, kind, n, data, w)
        _check_rows(base, _want(kind, rows, w), kind, f"benchmark form {kind}")
        before = total.value

        def c_form(pin, pout, pw):
            if kind == "inverse":
                rc = st.lib().smfft_istft_benchmark(pin, pout, pw, n, C * F, ctypes.byref(total))
            else:
                rc = st.lib().smfft_stft_benchmark(pin, pout, pw, n, C, F, hop, stride, int(kind == "power"), ctypes.byref(total))
            assert rc == 0 and total.value > before

        def mirror(pin, pout, pw):
            if kind == "inverse":
                status, ms = st.istft_benchmark(pin, pout, pw, n, C * F)
            else:
                status, ms = st.stft_benchmark(pin, pout, pw, n, C, F, hop, stride, power=kind == "power")
            assert status == 0 and ms > 0.0
        for form in (c_form, mirror):
            assert np.array_equal(rh.bits(_run(sm, st, kind, n, data, w, launch=form)), rh.bits(base)), (kind, form.__name__)


_TENSOR_SCRIPT = r"""
import sys
import numpy as np
import torch                                  # first: torch initialises the HIP runtime before the library uses it
torch.cuda.init()
sys.path.insert(0, sys.argv[1])
import smfft_amd as sm
from smfft_amd import stft as st
sm.FFT_init()
L2, MX = float(sys.argv[2]), float(sys.argv[3])
rng = np.random.default_rng(8)
def rows(got, want, factor, what):
    # per frame: the last axis
    d = (got - want).reshape(-1, want.shape[-1])
    w = want.reshape(-1, want.shape[-1])
    l2 = (torch.linalg.norm(d, dim=1) / torch.linalg.norm(w, dim=1)).max().item()
    mx = (d.abs().amax(dim=1) / w.abs().amax(dim=1)).max().item()
    print(f"{what}: worst row relL2 = {l2:.3e}, max = {mx:.3e}")
    assert l2 <= factor * L2 and mx <= factor * MX, (what, l2, mx)
for n, hop in ((512, 128), (512, 129), (8192, 2048)):
    s = torch.from_numpy(rng.standard_normal((2, 7 * n + 13)).astype(np.float32)).cuda()
    w = st.hann(n, "cuda")
    assert w.is_cuda and w.dtype == torch.float32 and w.shape == (n,)
    w64, s64 = w.double(), s.double()
    for center in (False, True):
        want = torch.stft(s64, n, hop, window=w64, center=center, pad_mode="reflect", onesided=True, return_complex=True).transpose(-1, -2)
        X = st.stft(s, n, hop, w, center=center)
        P = st.spectrogram(s, n, hop, w, center=center)
        assert X.shape == want.shape and X.dtype == torch.complex64 and X.is_cuda and X.is_contiguous()
        assert P.shape == want.shape and P.dtype == torch.float32
        assert X.shape[1] == st.frames(s.shape[1] + (n if center else 0), n, hop)
        torch.cuda.synchronize()
        rows(X.to(torch.complex128), want, 1.0, f"n={n} hop={hop} center={center} stft against torch.stft")
        rows(P.double(), want.abs() ** 2, 2.0, f"n={n} hop={hop} center={center} spectrogram against |torch.stft|^2")
        assert torch.equal(st.stft(s, n, hop, w, power=True, center=center).view(torch.int32), P.view(torch.int32))
    # one stream as a vector; no window
    X1 = st.stft(s[0], n, hop)
    want = torch.stft(s64[0], n, hop, window=torch.ones(n, dtype=torch.float64, device="cuda"), center=False, return_complex=True).transpose(-1, -2)
    assert X1.shape == (1,) + tuple(want.shape)
    rows(X1[0].to(torch.complex128), want, 1.0, f"n={n} hop={hop} one stream, no window")
    # the inverse frames are torch.fft.irfft times the window, and istft undoes stft(center=True) as torch.istft does
    X = st.stft(s, n, hop, w, center=True)
    y = st.istft_frames(X, w)
    assert y.shape == X.shape[:-1] + (n,) and y.dtype == torch.float32
    rows(y.double(), torch.fft.irfft(X.to(torch.complex128), n) * w64, 1.0, f"n={n} hop={hop} istft_frames against irfft x window")
    back = st.istft(X, hop, w, length=s.shape[1], center=True)
    tback = torch.istft(X.to(torch.complex128).transpose(-1, -2), n, hop, window=w64, center=True, length=s.shape[1])
    assert back.shape == s.shape
    if hop == n // 4:
        # (away from the last frames, which the signal's last 13 samples only half fill)
        cut = s.shape[1] - n
        rows(back[:, :cut].double(), tback[:, :cut], 2.0, f"n={n} hop={hop} istft against torch.istft")
        rows(back[:, :cut].double(), s64[:, :cut], 2.0, f"n={n} hop={hop} istft(stft(s)) against s")
    plain = st.overlap_add(y, hop)
    ref = torch.zeros_like(plain)
    for f in range(y.shape[1]):
        ref[:, f * hop:f * hop + n] += y[:, f]
    assert plain.shape == (2, (y.shape[1] - 1) * hop + n) and torch.allclose(plain, ref, rtol=0, atol=1e-5)
def refused(exc, f, *a, **k):
    try:
        f(*a, **k)
    except exc:
        return
    raise SystemExit(f"{f.__name__} was not refused with {exc.__name__}")
t = torch.zeros(2, 4096, device="cuda")
refused(TypeError, st.stft, t.double(), 512, 128)
refused(ValueError, st.stft, t[:, ::2], 512, 128)
refused(ValueError, st.stft, t, 500, 128)
refused(ValueError, st.stft, t, 512, 128, st.hann(512))                  # a window on another device
refused(ValueError, st.stft, t, 512, 128, st.hann(1024, "cuda"))
refused(ValueError, st.istft_frames, torch.zeros(2, 256, dtype=torch.complex64, device="cuda"))
refused(ValueError, st.istft, st.stft(t, 512, 128), 128, st.hann(512, "cuda"))     # Hann starts at zero: the envelope does too
print("ok")
"""


def test_tensors_on_the_device(st):
    """smfft_amd.stft on torch tensors on the device, in a process of its own in which torch initialises the HIP runtime before the
    library uses it (the order of tests/test_large_gpu.py): stft and spectrogram with center False and True against torch.stft (in
    fp64) on the device tensor, transposed, at n = 512 (hop 128 and an odd 129) and 8192; istft_frames against torch.fft.irfft times
    the window; istft against torch.istft and against the signal; overlap_add against the sum of the frames; tensors that are not
    contiguous float32, windows of another length or device and a window whose envelope reaches zero are refused"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _TENSOR_SCRIPT, root, repr(ROW_REL_L2), repr(ROW_MAX)], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("ok"), p.stdout + p.stderr
    assert ROW_REL_L2 == 1e-6 and ROW_MAX == 5e-6

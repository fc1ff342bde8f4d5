"""The polyphase filter bank channelizer for real streams on an MI355X (smfft_pfb_real_*, smfft_amd.pfb_real) against the fp64 model of
tools/pfb_real_model.py: both modes at every length over a grid of taps per channel, prototypes, streams and frames; a bare R2C at the
library's per-FFT bounds; agreement with the shipped complex bank at 2N channels; bit-identity across schedules and across stream
splits; a caller's stream, the benchmark form, interior pointers; the host conveniences on two tones.

Every run goes through _run (the harness of tests/test_pfb_gpu.py on float signals): the output is prefilled with 0xFF (NaN) and followed
by a 4096-element guard of 0x5A that must stay untouched; the signal buffer carries NaN in 4096 floats before stream 0, after stream
C - 1, and in every stream's unread tail [(F + P - 1) 2N, L), so that a read outside the contract shows up as a non-finite output.

Tolerances, per output spectrum (one (c, f) row): the complex bank's metrics and bounds (tests/test_pfb_gpu.py) with the frame's 2N real
samples in the place of its N complex ones.  With s[n] = sum_p |h[2 p N + n]| |x[(f + p) 2N + n]|, n < 2N, the scale the fp32
accumulation rounds at (by Parseval the whole 2N-point spectrum has norm <= sqrt(2N) ||s||, and its N + 1 output values no more):
  complex mode, on the N + 1 values X[0 ... N]: ||got - ref||_2 / (sqrt(2N) ||s||_2) <= 1e-6  and
                max|got - ref| / max(max|ref|, ||s||_2) <= 5e-6;
  power mode, Gaussian signals, on the N values: ||got - ref||_1 / ||ref||_1 <= 2e-6 and max|got - ref| / max(ref) <= 1e-5;
  power mode, tones (the branches of an off-centre tone cancel): the same derivation before its last step, as in tests/test_pfb_gpu.py.
Element 0 of every row is checked on its own as well: both of its components against (X[0], X[N]) within the row's max bound, and the
DC power against X[0]^2 within the row's power max bound.
A sequential fp32 emulation (weighted sum, complex64 FFT of the packed sequence, split in complex64; 2N in {512, 2048, 8192}, P in
{1, 4, 32}, Gaussian signal, Hamming-sinc prototype) stays at 9.6e-8, 2.1e-7, 1.9e-7 and 3.5e-7 of these four."""
import ctypes
import os
import sys

import numpy as np
import pytest

from oracle.np_reference import MAX_ABS_TOL, REL_L2_TOL, assert_close_fp32

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import pfb_model as pm  # noqa: E402
import pfb_real_model as prm  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [256, 512, 1024, 2048, 4096]
TAPS = [1, 2, 4, 8, 16, 32]
ROW_REL_L2, ROW_MAX = 1e-6, 5e-6
POWER_L1, POWER_MAX = 2e-6, 1e-5
GUARD = 4096                   # floats around the signal that are NaN, elements after the output that must stay untouched
worst = {"l2": 0.0, "max": 0.0, "pl1": 0.0, "pmax": 0.0}


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def pr():
    from smfft_amd import pfb_real
    pfb_real.lib()
    yield pfb_real
    print(f"\nworst seen: complex relL2 {worst['l2']:.3e} (bound {ROW_REL_L2}), max {worst['max']:.3e} (bound {ROW_MAX}); "
          f"power L1 {worst['pl1']:.3e} (bound {POWER_L1}), max {worst['pmax']:.3e} (bound {POWER_MAX})")


def _rand(rng, shape):
    return rng.standard_normal(shape).astype(np.float32)


def _prototypes(pr, rng, N, P):
    return {"windowed sinc": pr.prototype(N, P), "gaussian": rng.standard_normal(2 * P * N).astype(np.float32), "ones": np.ones(2 * P * N, np.float32)}


def _length(N, P, F, tail):
    """floats of a stream with F frames and `tail` (even, < 2N) unread ones"""
    assert tail % 2 == 0 and tail < 2 * N
    return (F + P - 1) * 2 * N + tail


def _signal_with_nans(x, N, P):
    """the device image of x (C, L): NaN in GUARD floats before and after, and in every stream's unread tail"""
    C, L = x.shape
    used = (prm.frames(L, N, P) + P - 1) * 2 * N
    body = x.copy()
    body[:, used:] = np.nan
    nan = np.full(GUARD, np.nan, np.float32)
    return np.concatenate([nan, body.reshape(-1), nan])


def _run(sm, pr, x, h, N, power, launcher=None, in_off=0, tap_off=0, out_off=0, finite=True):
    """launch through the device-pointer API (launcher(d_signal, L, C, d_taps, N, P, d_output, power) or pr.launch) from a signal
    fenced with NaN into an output fenced with a guard; returns the (C, F, N) result as the device wrote it after checking that the
    guard is untouched and nothing of the prefill is left.  in_off / tap_off (floats) and out_off (output elements) shift the three
    pointers into their buffers.  finite=False is for runs whose inputs hold NaN or Inf on purpose (tests/test_pfb_probes_gpu.py): the guards
    are checked all the same, the output may be non-finite."""
    C, L = x.shape
    P = h.size // (2 * N)
    F = prm.frames(L, N, P)
    width, dtype = (4, np.float32) if power else (8, np.complex64)
    image = _signal_with_nans(x, N, P)
    if in_off:
        image = np.concatenate([np.full(in_off, np.nan, np.float32), image])
    dx = sm.DeviceBuffer.from_host(image)
    dh = sm.DeviceBuffer.from_host(np.concatenate([np.full(tap_off, np.nan, np.float32), h]))
    total = C * F * N
    dout = sm.DeviceBuffer((out_off + total + GUARD) * width)
    if out_off:
        assert sm.lib.smfft_memset(dout.ptr, 0x5A, out_off * width) == 0
    assert sm.lib.smfft_memset(dout.ptr + out_off * width, 0xFF, total * width) == 0
    assert sm.lib.smfft_memset(dout.ptr + (out_off + total) * width, 0x5A, GUARD * width) == 0
    args = (dx.ptr + (in_off + GUARD) * 4, L, C, dh.ptr + tap_off * 4, N, P, dout.ptr + out_off * width)
    if launcher is None:
        pr.launch(*args, power=power)
    else:
        launcher(*args, power)
    assert sm.lib.smfft_synchronize() == 0
    raw = dout.to_host(np.uint8, ((out_off + total + GUARD) * width,))
    assert np.all(raw[:out_off * width] == 0x5A), "the kernel wrote before its output"
    assert np.all(raw[(out_off + total) * width:] == 0x5A), "the kernel wrote past its output"
    out = raw[out_off * width:(out_off + total) * width].view(dtype).reshape(C, F, N)
    assert not finite or np.all(np.isfinite(out.view(np.float32))), "outputs left unwritten, or a sample read outside the contract"
    for b in (dx, dh, dout):
        b.free()
    return out


def _unpack(packed):
    out = np.empty(packed.shape[:-1] + (packed.shape[-1] + 1,), np.complex128)
    out[..., :-1] = packed
    out[..., 0] = packed[..., 0].real
    out[..., -1] = packed[..., 0].imag
    return out


def _check_complex(got, ref, s, what):
    """got: (C, F, N) packed rows of the device, ref: (C, F, N + 1) rfft rows, s: (C, F, 2N) the accumulation's scale"""
    N = got.shape[-1]
    assert ref.shape == got.shape[:-1] + (N + 1,) and s.shape == got.shape[:-1] + (2 * N,)
    d = _unpack(got) - ref
    sn = np.linalg.norm(s, axis=-1)
    l2 = np.linalg.norm(d, axis=-1) / np.maximum(np.sqrt(2 * N) * sn, 1e-300)
    denom = np.maximum(np.maximum(np.abs(ref).max(axis=-1), sn), 1e-300)
    mx = np.abs(d).max(axis=-1) / denom
    # element 0 on its own: (X[0], X[N]), both real
    e0 = np.maximum(np.abs(got[..., 0].real.astype(np.float64) - ref[..., 0].real), np.abs(got[..., 0].imag.astype(np.float64) - ref[..., N].real)) / denom
    print(f"{what}: relL2 {l2.max():.3e} max {mx.max():.3e} element 0 {e0.max():.3e}")
    worst["l2"], worst["max"] = max(worst["l2"], l2.max()), max(worst["max"], mx.max())
    assert l2.max() <= ROW_REL_L2 and mx.max() <= ROW_MAX and e0.max() <= ROW_MAX, f"{what}: relL2={l2.max():.3e} max={mx.max():.3e} element 0={e0.max():.3e}"


def _check_power(got, ref, what):
    """got: (C, F, N) powers of the device, ref: (C, F, N + 1) rfft rows"""
    refp = prm.power(ref)
    d = np.abs(got.astype(np.float64) - refp)
    l1 = d.sum(axis=-1) / refp.sum(axis=-1)
    mx = d.max(axis=-1) / refp.max(axis=-1)
    e0 = np.abs(got[..., 0].astype(np.float64) - ref[..., 0].real ** 2) / refp.max(axis=-1)       # DC alone: X[0]^2, no Nyquist in it
    print(f"{what}: L1 {l1.max():.3e} max {mx.max():.3e} element 0 {e0.max():.3e}")
    worst["pl1"], worst["pmax"] = max(worst["pl1"], l1.max()), max(worst["pmax"], mx.max())
    assert l1.max() <= POWER_L1 and mx.max() <= POWER_MAX and e0.max() <= POWER_MAX, f"{what}: L1={l1.max():.3e} max={mx.max():.3e} element 0={e0.max():.3e}"


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("P", TAPS)
def test_filter_bank_matches_the_model(sm, pr, N, P):
    """every prototype x (C, F) in {(1, 1), (1, 4096/N + 1), (3, 2 4096/N + 1), (2, 300)} (one frame; a partial second tile; tiles
    straddling streams; many tiles), ragged even tails, both modes, Gaussian signals"""
    rng = np.random.default_rng(1000 * N + P)
    per = 4096 // N
    protos = _prototypes(pr, rng, N, P)
    for C, F, tail in ((1, 1, 0), (1, per + 1, 2 * N - 2), (3, 2 * per + 1, N + 6), (2, 300, 18)):
        L = _length(N, P, F, tail)
        x = _rand(rng, (C, L))
        for name, h in protos.items():
            ref, s = prm.pfb_real(x, h, N), prm.scale(x, h, N)
            assert ref.shape == (C, F, N + 1)
            what = f"N={N} P={P} {name} C={C} F={F}"
            _check_complex(_run(sm, pr, x, h, N, False), ref, s, what)
            _check_power(_run(sm, pr, x, h, N, True), ref, what + " power")


@pytest.mark.parametrize("N", SIZES)
def test_one_tap_of_ones_is_a_bare_r2c(sm, pr, N):
    """P = 1, h = 1: np.fft.rfft of every frame at the library's per-FFT bounds (oracle/np_reference.py)"""
    rng = np.random.default_rng(N)
    F = 3 * (4096 // N) + 1
    x = _rand(rng, (2, F * 2 * N + 6))
    got = _unpack(_run(sm, pr, x, np.ones(2 * N, np.float32), N, False))
    want = np.fft.rfft(x[:, :F * 2 * N].astype(np.float64).reshape(2, F, 2 * N), axis=-1)
    l2, mx = assert_close_fp32(got.reshape(-1, N + 1), want.reshape(-1, N + 1), f"real PFB P=1 h=1 N={N}")
    print(f"N={N}: relL2 {l2:.3e} (tol {REL_L2_TOL}) max {mx:.3e} (tol {MAX_ABS_TOL})")


@pytest.mark.parametrize("N", [256, 512, 1024, 2048])
def test_agrees_with_the_complex_bank_of_2n_channels(sm, pr, N):
    """channels 1 ... N - 1 against smfft_pfb_launch with 2N channels on x + 0j, within the sum of both kernels' bounds (each is within
    its own of the fp64 model, and the two models are the same numbers: tests/test_pfb_real_cpu.py)"""
    from smfft_amd import pfb
    rng = np.random.default_rng(3 * N)
    P, C, F = 4, 2, 4096 // N + 3
    x, h = _rand(rng, (C, _length(N, P, F, 10))), pr.prototype(N, P)
    got = _run(sm, pr, x, h, N, False)
    other = pfb.channelize(x.astype(np.complex64), h, 2 * N)
    assert other.shape == (C, F, 2 * N)
    d = got[..., 1:].astype(np.complex128) - other[..., 1:N]
    ref, sn = prm.pfb_real(x, h, N), np.linalg.norm(prm.scale(x, h, N), axis=-1)
    l2 = np.linalg.norm(d, axis=-1) / (np.sqrt(2 * N) * sn)
    mx = np.abs(d).max(axis=-1) / np.maximum(np.abs(ref).max(axis=-1), sn)
    print(f"N={N}: against the complex bank relL2 {l2.max():.3e} (bound {2 * ROW_REL_L2}) max {mx.max():.3e} (bound {2 * ROW_MAX})")
    assert l2.max() <= 2 * ROW_REL_L2 and mx.max() <= 2 * ROW_MAX


# ------------------------------------------------------------------------------------------------ bit identity
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("N,P,power", [(1024, 8, False), (4096, 4, True), (256, 16, False)])
def test_every_schedule_gives_the_same_bits(sm, pr, N, P, power):
    """3000 tiles: more runs than any grid for R = 1 and 3 (the outer stride runs), fewer for 16, one run for R above the tile count"""
    rng = np.random.default_rng(N + P)
    tiles = 3000
    F = tiles * (4096 // N) - 1
    L = _length(N, P, F, 10)
    x, h = _rand(rng, (1, L)), pr.prototype(N, P)
    base = _run(sm, pr, x, h, N, power)
    for R in (1, 3, 16, tiles + 7):
        got = _run(sm, pr, x, h, N, power, launcher=lambda *a, R=R: pr.launch_tuned(*a[:-1], R, power=a[-1]))
        assert np.array_equal(_bits(got), _bits(base)), f"N={N} P={P} R={R}"
    # and they are right: the first and the last frames against the model
    for f0 in (0, F - 8):
        xs = x[:, f0 * 2 * N:(f0 + 8 + P - 1) * 2 * N]
        ref = prm.pfb_real(xs, h, N)
        if power:
            _check_power(base[:, f0:f0 + 8], ref, f"schedules N={N} frames {f0}...")
        else:
            _check_complex(base[:, f0:f0 + 8], ref, prm.scale(xs, h, N), f"schedules N={N} frames {f0}...")


@pytest.mark.parametrize("N,P", [(512, 4), (2048, 2)])
def test_three_streams_equal_three_launches(sm, pr, N, P):
    rng = np.random.default_rng(N)
    F = 2 * (4096 // N) + 1                       # tiles straddle the streams
    x, h = _rand(rng, (3, _length(N, P, F, 6))), rng.standard_normal(2 * P * N).astype(np.float32)
    for power in (False, True):
        together = _run(sm, pr, x, h, N, power)
        for c in range(3):
            alone = _run(sm, pr, x[c:c + 1], h, N, power)
            assert np.array_equal(_bits(alone[0]), _bits(together[c])), (N, P, power, c)


# ------------------------------------------------------------------------------------------------ the ABI's corners
def test_caller_stream(sm, pr):
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value
    rng = np.random.default_rng(11)
    N, P, C, F = 1024, 8, 2, 37
    x, h = _rand(rng, (C, _length(N, P, F, 100))), pr.prototype(N, P)

    def on_stream(*a):
        pr.launch(*a[:-1], power=a[-1], stream=stream.value)
        assert hip.hipStreamSynchronize(stream) == 0

    ref = prm.pfb_real(x, h, N)
    _check_complex(_run(sm, pr, x, h, N, False, launcher=on_stream), ref, prm.scale(x, h, N), "caller's stream")
    _check_power(_run(sm, pr, x, h, N, True, launcher=on_stream), ref, "caller's stream, power")
    assert hip.hipStreamDestroy(stream) == 0


def test_benchmark_adds_to_its_total(sm, pr):
    rng = np.random.default_rng(12)
    N, P, C, F = 2048, 4, 1, 300
    x, h = _rand(rng, (C, _length(N, P, F, 2))), pr.prototype(N, P)
    seen = []

    def timed(*a):
        d_signal, L, C_, d_taps, N_, P_, d_output, power = a
        t = ctypes.c_double(5.0)
        assert pr.lib().smfft_pfb_real_benchmark(d_signal, L, C_, d_taps, N_, P_, int(power), d_output, ctypes.byref(t)) == 0
        first = t.value
        assert first > 5.0
        assert pr.lib().smfft_pfb_real_benchmark(d_signal, L, C_, d_taps, N_, P_, int(power), d_output, ctypes.byref(t)) == 0
        assert t.value > first
        rc, ms = pr.benchmark(d_signal, L, C_, d_taps, N_, P_, d_output, power=power)
        assert rc == 0 and ms > 0.0
        seen.append(ms)

    _check_complex(_run(sm, pr, x, h, N, False, launcher=timed), prm.pfb_real(x, h, N), prm.scale(x, h, N), "benchmark form")
    assert len(seen) == 1


def test_interior_pointers(sm, pr):
    """signal and taps an even number of floats inside their buffers (8-byte aligned), the output at odd element offsets (8-byte
    aligned in complex mode, 4 in power mode)"""
    rng = np.random.default_rng(13)
    for N, P in ((256, 4), (4096, 2)):
        x, h = _rand(rng, (2, _length(N, P, 4096 // N + 2, 6))), rng.standard_normal(2 * P * N).astype(np.float32)
        ref = prm.pfb_real(x, h, N)
        _check_complex(_run(sm, pr, x, h, N, False, in_off=6, tap_off=2, out_off=5), ref, prm.scale(x, h, N), f"interior N={N}")
        _check_power(_run(sm, pr, x, h, N, True, in_off=2, tap_off=10, out_off=1), ref, f"interior N={N} power")


# ------------------------------------------------------------------------------------------------ the host conveniences
def _leakage(power, channel):
    power = np.asarray(power, np.float64)
    return (power.sum(axis=-1) - power[..., channel]) / power[..., channel]


@pytest.mark.parametrize("N", [256, 1024, 4096])
def test_channelize_and_prototype_on_two_tones(sm, pr, N):
    """a unit cosine at channel 100.37 plus one of a tenth of its amplitude at channel N/2 + 7.5 (channel k = k cycles per 2N samples),
    through prototype() and channelize(): parity with the model in all three output forms, and the strong tone alone leaks less from
    the device's power output than from the rectangular window of a plain rfft of one frame, the less the longer the prototype"""
    t = np.arange(40 * 2 * N + 26)
    strong = np.cos(2 * np.pi * 100.37 * t / (2 * N))
    both = (strong + 0.1 * np.cos(2 * np.pi * (N / 2 + 7.5) * t / (2 * N))).astype(np.float32)
    rect = _leakage(np.abs(np.fft.rfft(strong[:2 * N].astype(np.float32).astype(np.float64))[:N]) ** 2, 100)
    leaks = []
    for P in (2, 4, 8, 16, 32):
        h = pr.prototype(N, P)
        assert h.dtype == np.float32 and h.shape == (2 * P * N,)
        ref, s = prm.pfb_real(both, h, N), prm.scale(both, h, N)
        got = pr.channelize(both, h, N)
        assert got.shape == ref.shape == (1, 41 - P, N + 1) and got.dtype == np.complex64
        packed = pr.channelize(both, h, N, packed=True)
        assert packed.shape == (1, 41 - P, N) and packed.dtype == np.complex64
        assert np.array_equal(_bits(pr.unpack(packed)), _bits(got)), "channelize unpacks what the device wrote"
        _check_complex(packed, ref, s, f"tones N={N} P={P}")
        gotp = pr.channelize(both, h, N, power=True)
        assert gotp.shape == (1, 41 - P, N) and gotp.dtype == np.float32
        refp = prm.power(ref)
        d = np.abs(gotp.astype(np.float64) - refp)
        yn, ym, sn = np.linalg.norm(ref, axis=-1), np.abs(ref).max(axis=-1), np.linalg.norm(s, axis=-1)
        l1 = d.sum(axis=-1) / (yn * np.sqrt(2 * N) * sn)
        mx = d.max(axis=-1) / (ym * np.maximum(ym, sn))
        print(f"tones N={N} P={P} power: L1 {l1.max():.3e} max {mx.max():.3e}")
        assert l1.max() <= POWER_L1 and mx.max() <= POWER_MAX, (N, P, l1.max(), mx.max())
        leak = _leakage(pr.channelize(strong.astype(np.float32), h, N, power=True), 100)
        print(f"tones N={N} P={P}: leakage {leak.max():.3g} against {rect:.3g} of the plain transform")
        assert leak.max() < rect, (N, P, leak.max(), rect)
        leaks.append(leak.max())
    assert all(b < a for a, b in zip(leaks, leaks[1:])), leaks

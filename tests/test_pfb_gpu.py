"""The polyphase filter bank channelizer on an MI355X (smfft_pfb_*, smfft_amd.pfb) against the fp64 model of tools/pfb_model.py: both
modes at every length over a grid of taps per channel, prototypes, streams and frames; a bare transform at the library's per-FFT
bounds; bit-identity across schedules and across stream splits; a caller's stream, the benchmark form, interior pointers, 64-bit
offsets; the host conveniences on two tones.

Every run goes through _run: the output is prefilled with 0xFF (NaN) and followed by a 4096-element guard of 0x5A that must stay
untouched; the signal buffer carries 0xFF -- NaN -- in 4096 elements before stream 0, after stream C - 1, and in every stream's unread
tail [(F + P - 1) N, L) (the tail belongs to its own stream, so this never touches another stream's frames), so that a read outside
the contract shows up as a non-finite output.

Tolerances, per output spectrum (one (c, f) row of N values).  With s[n] = sum_p |h[p N + n]| |x[(f + p) N + n]|, the scale the fp32
accumulation rounds at (by Parseval ||y_f|| <= sqrt(N) ||s||, with equality when the taps do not cancel):
  complex mode: ||got - ref||_2 / (sqrt(N) ||s||_2) <= 1e-6  and  max|got - ref| / max(max|ref|, ||s||_2) <= 5e-6 -- the FIR rows'
                bounds (tests/test_fir_gpu.py), sized for two transforms and a product: room for one transform plus a 32-term sum;
  power mode, Gaussian signals (no cancellation): ||got - ref||_1 / ||ref||_1 <= 2e-6 and max|got - ref| / max(ref) <= 1e-5 -- twice the
                amplitude bounds, since | |y + d|^2 - |y|^2 | <= 2 |y| |d| + |d|^2 and sum |y| |d| <= ||y||_2 ||d||_2.
  power mode, tones (test_channelize_and_prototype_on_two_tones; the P branches of an off-centre tone do cancel, so sqrt(N) ||s|| exceeds
                ||y||): the same derivation before its last step, ||got - ref||_1 <= 2e-6 ||y||_2 sqrt(N) ||s||_2 and
                max|got - ref| <= 1e-5 max|y| max(max|y|, ||s||_2); without cancellation these are the two bounds above."""
import ctypes
import os
import sys

import numpy as np
import pytest

from oracle.np_reference import MAX_ABS_TOL, REL_L2_TOL, assert_close_fp32

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import pfb_model as pm  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [256, 512, 1024, 2048, 4096]
TAPS = [1, 2, 4, 8, 16, 32]
ROW_REL_L2, ROW_MAX = 1e-6, 5e-6
POWER_L1, POWER_MAX = 2e-6, 1e-5
GUARD = 4096                   # elements around the signal that are NaN, elements after the output that must stay untouched
worst = {"l2": 0.0, "max": 0.0, "pl1": 0.0, "pmax": 0.0}


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def pfb():
    from smfft_amd import pfb
    pfb.lib()
    yield pfb
    print(f"\nworst seen: complex relL2 {worst['l2']:.3e} (bound {ROW_REL_L2}), max {worst['max']:.3e} (bound {ROW_MAX}); "
          f"power L1 {worst['pl1']:.3e} (bound {POWER_L1}), max {worst['pmax']:.3e} (bound {POWER_MAX})")


def _rand(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def _prototypes(pfb, rng, N, P):
    return {"windowed sinc": pfb.prototype(N, P), "gaussian": rng.standard_normal(P * N).astype(np.float32), "ones": np.ones(P * N, np.float32)}


def _length(N, P, F, tail):
    return (F + P - 1) * N + tail


def _signal_with_nans(x, N, P):
    """the device image of x (C, L): NaN in GUARD elements before and after, and in every stream's unread tail"""
    C, L = x.shape
    used = (pm.frames(L, N, P) + P - 1) * N
    body = x.copy()
    body[:, used:] = np.nan + 1j * np.nan
    nan = np.full(GUARD, np.nan + 1j * np.nan, np.complex64)
    return np.concatenate([nan, body.reshape(-1), nan])


def _run(sm, pfb, x, h, N, power, launcher=None, in_off=0, tap_off=0, out_off=0, finite=True):
    """launch through the device-pointer API (launcher(d_signal, L, C, d_taps, N, P, d_output, power) or pfb.launch) from a signal
    fenced with NaN into an output fenced with a guard; returns the (C, F, N) result after checking that the guard is untouched and
    nothing of the prefill is left.  The *_off arguments shift the three pointers by that many elements into their buffers.
    finite=False is for runs whose inputs hold NaN or Inf on purpose (tests/test_pfb_probes_gpu.py): the guards are checked all the same, the
    output may be non-finite."""
    C, L = x.shape
    P = h.size // N
    F = pm.frames(L, N, P)
    width, dtype = (4, np.float32) if power else (8, np.complex64)
    image = _signal_with_nans(x, N, P)
    if in_off:
        image = np.concatenate([np.full(in_off, np.nan + 1j * np.nan, np.complex64), image])
    dx = sm.DeviceBuffer.from_host(image)
    dh = sm.DeviceBuffer.from_host(np.concatenate([np.full(tap_off, np.nan, np.float32), h]))
    total = C * F * N
    dout = sm.DeviceBuffer((out_off + total + GUARD) * width)
    if out_off:
        assert sm.lib.smfft_memset(dout.ptr, 0x5A, out_off * width) == 0
    assert sm.lib.smfft_memset(dout.ptr + out_off * width, 0xFF, total * width) == 0
    assert sm.lib.smfft_memset(dout.ptr + (out_off + total) * width, 0x5A, GUARD * width) == 0
    args = (dx.ptr + (in_off + GUARD) * 8, L, C, dh.ptr + tap_off * 4, N, P, dout.ptr + out_off * width)
    if launcher is None:
        pfb.launch(*args, power=power)
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


def _check_complex(got, ref, s, what):
    """got, ref: (C, F, N) spectra, s: (C, F, N) the accumulation's scale"""
    N = ref.shape[-1]
    d = got.astype(np.complex128) - ref
    sn = np.linalg.norm(s, axis=-1)
    l2 = np.linalg.norm(d, axis=-1) / np.maximum(np.sqrt(N) * sn, 1e-300)
    mx = np.abs(d).max(axis=-1) / np.maximum(np.maximum(np.abs(ref).max(axis=-1), sn), 1e-300)
    print(f"{what}: relL2 {l2.max():.3e} max {mx.max():.3e}")
    worst["l2"], worst["max"] = max(worst["l2"], l2.max()), max(worst["max"], mx.max())
    assert l2.max() <= ROW_REL_L2 and mx.max() <= ROW_MAX, f"{what}: relL2={l2.max():.3e} max={mx.max():.3e}"


def _check_power(got, ref, what):
    d = np.abs(got.astype(np.float64) - ref)
    l1 = d.sum(axis=-1) / ref.sum(axis=-1)
    mx = d.max(axis=-1) / ref.max(axis=-1)
    print(f"{what}: L1 {l1.max():.3e} max {mx.max():.3e}")
    worst["pl1"], worst["pmax"] = max(worst["pl1"], l1.max()), max(worst["pmax"], mx.max())
    assert l1.max() <= POWER_L1 and mx.max() <= POWER_MAX, f"{what}: L1={l1.max():.3e} max={mx.max():.3e}"


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("P", TAPS)
def test_filter_bank_matches_the_model(sm, pfb, N, P):
    """every prototype x (C, F) in {(1, 1), (1, 4096/N + 1), (3, 2 4096/N + 1), (2, 1000)} (one frame; a partial second tile; tiles
    straddling streams; many tiles), ragged tails, both modes, Gaussian signals"""
    rng = np.random.default_rng(1000 * N + P)
    per = 4096 // N
    protos = _prototypes(pfb, rng, N, P)
    for C, F, tail in ((1, 1, 0), (1, per + 1, N - 1), (3, 2 * per + 1, N // 2 + 3), (2, 1000, 17)):
        L = _length(N, P, F, tail)
        x = _rand(rng, (C, L))
        for name, h in protos.items():
            ref, s = pm.pfb(x, h, N), pm.scale(x, h, N)
            assert ref.shape == (C, F, N)
            what = f"N={N} P={P} {name} C={C} F={F}"
            _check_complex(_run(sm, pfb, x, h, N, False), ref, s, what)
            _check_power(_run(sm, pfb, x, h, N, True), ref.real ** 2 + ref.imag ** 2, what + " power")


@pytest.mark.parametrize("N", SIZES)
def test_one_tap_of_ones_is_a_bare_transform(sm, pfb, N):
    """P = 1, h = 1: the library's per-FFT bounds (oracle/np_reference.py)"""
    rng = np.random.default_rng(N)
    F = 3 * (4096 // N) + 1
    x = _rand(rng, (2, F * N + 5))
    got = _run(sm, pfb, x, np.ones(N, np.float32), N, False)
    want = np.fft.fft(x[:, :F * N].astype(np.complex128).reshape(2, F, N), axis=-1)
    l2, mx = assert_close_fp32(got.reshape(-1, N), want.reshape(-1, N), f"PFB P=1 h=1 N={N}")
    print(f"N={N}: relL2 {l2:.3e} (tol {REL_L2_TOL}) max {mx:.3e} (tol {MAX_ABS_TOL})")


# ------------------------------------------------------------------------------------------------ bit identity
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("N,P,power", [(1024, 8, False), (4096, 4, True), (256, 16, False)])
def test_every_schedule_gives_the_same_bits(sm, pfb, N, P, power):
    """15000 tiles: more runs than any grid for R = 1, 3 and 16 (the outer stride runs), one run for R above the tile count"""
    rng = np.random.default_rng(N + P)
    tiles = 15000
    F = tiles * (4096 // N) - 1
    L = _length(N, P, F, 9)
    x, h = _rand(rng, (1, L)), pfb.prototype(N, P)
    base = _run(sm, pfb, x, h, N, power)
    for R in (1, 3, 16, tiles + 7):
        got = _run(sm, pfb, x, h, N, power, launcher=lambda *a, R=R: pfb.launch_tuned(*a[:-1], R, power=a[-1]))
        assert np.array_equal(_bits(got), _bits(base)), f"N={N} P={P} R={R}"
    # and they are right: the first and the last frames against the model
    for f0 in (0, F - 8):
        xs = x[:, f0 * N:(f0 + 8 + P - 1) * N]
        ref = pm.pfb(xs, h, N)
        if power:
            _check_power(base[:, f0:f0 + 8], ref.real ** 2 + ref.imag ** 2, f"schedules N={N} frames {f0}...")
        else:
            _check_complex(base[:, f0:f0 + 8], ref, pm.scale(xs, h, N), f"schedules N={N} frames {f0}...")


@pytest.mark.parametrize("N,P", [(512, 4), (2048, 2)])
def test_three_streams_equal_three_launches(sm, pfb, N, P):
    rng = np.random.default_rng(N)
    F = 2 * (4096 // N) + 1                       # tiles straddle the streams
    x, h = _rand(rng, (3, _length(N, P, F, 5))), rng.standard_normal(P * N).astype(np.float32)
    for power in (False, True):
        together = _run(sm, pfb, x, h, N, power)
        for c in range(3):
            alone = _run(sm, pfb, x[c:c + 1], h, N, power)
            assert np.array_equal(_bits(alone[0]), _bits(together[c])), (N, P, power, c)


# ------------------------------------------------------------------------------------------------ the ABI's corners
def test_caller_stream(sm, pfb):
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value
    rng = np.random.default_rng(11)
    N, P, C, F = 1024, 8, 2, 37
    x, h = _rand(rng, (C, _length(N, P, F, 100))), pfb.prototype(N, P)

    def on_stream(*a):
        pfb.launch(*a[:-1], power=a[-1], stream=stream.value)
        assert hip.hipStreamSynchronize(stream) == 0

    _check_complex(_run(sm, pfb, x, h, N, False, launcher=on_stream), pm.pfb(x, h, N), pm.scale(x, h, N), "caller's stream")
    _check_power(_run(sm, pfb, x, h, N, True, launcher=on_stream), pm.pfb(x, h, N, power=True), "caller's stream, power")
    assert hip.hipStreamDestroy(stream) == 0


def test_benchmark_adds_to_its_total(sm, pfb):
    rng = np.random.default_rng(12)
    N, P, C, F = 2048, 4, 1, 300
    x, h = _rand(rng, (C, _length(N, P, F, 1))), pfb.prototype(N, P)
    seen = []

    def timed(*a):
        d_signal, L, C_, d_taps, N_, P_, d_output, power = a
        t = ctypes.c_double(5.0)
        assert pfb.lib().smfft_pfb_benchmark(d_signal, L, C_, d_taps, N_, P_, int(power), d_output, ctypes.byref(t)) == 0
        first = t.value
        assert first > 5.0
        assert pfb.lib().smfft_pfb_benchmark(d_signal, L, C_, d_taps, N_, P_, int(power), d_output, ctypes.byref(t)) == 0
        assert t.value > first
        rc, ms = pfb.benchmark(d_signal, L, C_, d_taps, N_, P_, d_output, power=power)
        assert rc == 0 and ms > 0.0
        seen.append(ms)

    _check_complex(_run(sm, pfb, x, h, N, False, launcher=timed), pm.pfb(x, h, N), pm.scale(x, h, N), "benchmark form")
    assert len(seen) == 1


def test_interior_pointers(sm, pfb):
    """signal, taps and output at odd element offsets inside their buffers (8-byte aligned, 4 for taps and the power output)"""
    rng = np.random.default_rng(13)
    for N, P in ((256, 4), (4096, 2)):
        x, h = _rand(rng, (2, _length(N, P, 4096 // N + 2, 3))), rng.standard_normal(P * N).astype(np.float32)
        ref = pm.pfb(x, h, N)
        _check_complex(_run(sm, pfb, x, h, N, False, in_off=3, tap_off=1, out_off=5), ref, pm.scale(x, h, N), f"interior N={N}")
        _check_power(_run(sm, pfb, x, h, N, True, in_off=1, tap_off=3, out_off=1), ref.real ** 2 + ref.imag ** 2, f"interior N={N} power")


def test_offsets_beyond_two_to_the_31(sm, pfb):
    """N = 1024, P = 4, C = 2, F = 2^20 + 8: 2^31 + 22538 input elements and 2^31 + 16384 output elements in one launch (17 GiB in, 17 GiB
    out), complex mode.  The signal is made on the device: stream c is an uploaded Gaussian block of 2^24 + 1 elements repeated from a
    stream-dependent phase, x_c[i] = B[(i + 4099 c + 17) mod (2^24 + 1)] -- the block length is odd and every sampled window starts
    at another phase of it, so no two sampled windows are equal.  Sampled frames -- the first, the last, the two either side of output
    element 2^31 and the two either side of the stream boundary -- against the model on the input slice copied back."""
    N, P, C = 1024, 4, 2
    F = (1 << 20) + 8
    L = _length(N, P, F, 5)
    assert C * L > 1 << 31 and C * F * N > 1 << 31
    B = (1 << 24) + 1
    rng = np.random.default_rng(14)
    block = _rand(rng, (B,))
    h = pfb.prototype(N, P)
    dblock, dh = sm.DeviceBuffer.from_host(block), sm.DeviceBuffer.from_host(h)
    dx = sm.DeviceBuffer((C * L + 2 * GUARD) * 8)
    dout = sm.DeviceBuffer((C * F * N + GUARD) * 8)
    assert sm.lib.smfft_memset(dx.ptr, 0xFF, dx.nbytes) == 0
    for c in range(C):
        i, phase = 0, (4099 * c + 17) % B
        while i < L:
            n = min(B - phase, L - i)
            assert sm.lib.smfft_memcpy_d2d(dx.ptr + (GUARD + c * L + i) * 8, dblock.ptr + phase * 8, n * 8) == 0
            i, phase = i + n, 0
    assert sm.lib.smfft_memset(dout.ptr, 0xFF, C * F * N * 8) == 0
    assert sm.lib.smfft_memset(dout.ptr + C * F * N * 8, 0x5A, GUARD * 8) == 0
    pfb.launch(dx.ptr + GUARD * 8, L, C, dh.ptr, N, P, dout.ptr)
    assert sm.lib.smfft_synchronize() == 0
    guard = np.empty(GUARD * 8, np.uint8)
    assert sm.lib.smfft_memcpy_d2h(guard.ctypes.data, dout.ptr + C * F * N * 8, guard.nbytes) == 0
    assert np.all(guard == 0x5A), "the kernel wrote past its output"
    split = (1 << 31) // N                                   # the pair that holds output element 2^31
    pairs = [0, C * F - 1, split - 1, split, F - 1, F]
    assert F < split - 1 and split < C * F - 1
    seen = set()
    for g in pairs:
        c, f = divmod(g, F)
        xs = np.empty((1, P * N), np.complex64)
        assert sm.lib.smfft_memcpy_d2h(xs.ctypes.data, dx.ptr + (GUARD + c * L + f * N) * 8, xs.nbytes) == 0
        phase = (f * N + 4099 * c + 17) % B
        assert np.array_equal(xs[0], np.take(block, np.arange(phase, phase + P * N), mode="wrap")) and phase not in seen
        seen.add(phase)
        got = np.empty((1, 1, N), np.complex64)
        assert sm.lib.smfft_memcpy_d2h(got.ctypes.data, dout.ptr + g * N * 8, got.nbytes) == 0
        assert np.all(np.isfinite(got.view(np.float32)))
        _check_complex(got, pm.pfb(xs, h, N), pm.scale(xs, h, N), f"2^31: pair {g} (c={c}, f={f})")
    for b in (dblock, dh, dx, dout):
        b.free()


# ------------------------------------------------------------------------------------------------ the host conveniences
def _leakage(power, channel):
    power = np.asarray(power, np.float64)
    return (power.sum(axis=-1) - power[..., channel]) / power[..., channel]


@pytest.mark.parametrize("N", [256, 1024, 4096])
def test_channelize_and_prototype_on_two_tones(sm, pfb, N):
    """a unit tone at channel 100.37 plus one of a tenth of its amplitude at channel N/2 + 7.5, through prototype() and channelize(): parity
    with the model in both modes, and the strong tone alone leaks less from the device's power output than from the rectangular
    window of a plain transform of one frame (smfft_amd.c2c)"""
    t = np.arange(40 * N + 13)
    strong = np.exp(2j * np.pi * 100.37 * t / N)
    both = (strong + 0.1 * np.exp(2j * np.pi * (N / 2 + 7.5) * t / N)).astype(np.complex64)
    rect = np.abs(sm.c2c(strong[:N].astype(np.complex64)[None, :])[0].astype(np.complex128)) ** 2
    rect = _leakage(rect, 100)
    for P in (2, 4, 8, 16, 32):
        h = pfb.prototype(N, P)
        assert h.dtype == np.float32 and h.shape == (P * N,)
        ref, s = pm.pfb(both, h, N), pm.scale(both, h, N)
        got = pfb.channelize(both, h, N)
        assert got.shape == ref.shape == (1, 41 - P, N) and got.dtype == np.complex64
        _check_complex(got, ref, s, f"tones N={N} P={P}")
        gotp = pfb.channelize(both, h, N, power=True)
        assert gotp.shape == ref.shape and gotp.dtype == np.float32
        refp = ref.real ** 2 + ref.imag ** 2
        d = np.abs(gotp.astype(np.float64) - refp)
        yn, ym, sn = np.linalg.norm(ref, axis=-1), np.abs(ref).max(axis=-1), np.linalg.norm(s, axis=-1)
        l1 = d.sum(axis=-1) / (yn * np.sqrt(N) * sn)
        mx = d.max(axis=-1) / (ym * np.maximum(ym, sn))
        print(f"tones N={N} P={P} power: L1 {l1.max():.3e} max {mx.max():.3e}")
        assert l1.max() <= POWER_L1 and mx.max() <= POWER_MAX, (N, P, l1.max(), mx.max())
        leak = _leakage(pfb.channelize(strong.astype(np.complex64), h, N, power=True), 100)
        print(f"tones N={N} P={P}: leakage {leak.max():.3g} against {rect:.3g} of the plain transform")
        assert leak.max() < rect, (N, P, leak.max(), rect)

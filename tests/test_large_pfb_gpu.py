"""The polyphase filter bank channelizer for N = 8192 / 16384 channels on an MI355X (smfft_large_pfb_*, smfft_amd.large_pfb) against the
fp64 model of tools/large_pfb_model.py: both modes at both lengths over a grid of taps per channel, prototypes, streams and frames;
several rounds of a small grid under both schedules; more pairs than the device's grid; a bare transform at the library's per-FFT
bounds; bit-identity across schedules, grids and stream splits; a caller's stream, the benchmark form, interior pointers, 64-bit
offsets; the host conveniences on two tones.

Every run goes through tests/test_pfb_gpu.py's _run: the output is prefilled with 0xFF (NaN) and followed by a guard of 0x5A that must
stay untouched; the signal carries NaN before stream 0, after the last stream and in every stream's unread tail.  The bounds are that
file's row bounds (its docstring derives them): complex ||d||_2 / (sqrt(N) ||s||_2) <= 1e-6 and max <= 5e-6, power L1 <= 2e-6 and
max <= 1e-5.  An fp32 emulation on the CPU (sequential fp32 weighted sum, complex64 FFT; N in {8192, 16384}, P in {1, 8, 32}, Gaussian
and all-ones taps) stays at <= 3.7e-8, 9.1e-8, 1.2e-7 and 1.8e-7 of the four."""
import ctypes
import os
import sys

import numpy as np
import pytest

from oracle.np_reference import MAX_ABS_TOL, REL_L2_TOL, assert_close_fp32
from tests.test_pfb_gpu import GUARD, POWER_L1, POWER_MAX, ROW_MAX, ROW_REL_L2, _bits, _check_complex, _check_power, _length, _rand, _run
from tests.test_pfb_gpu import worst as _worst

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import large_pfb_model as lpm  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [8192, 16384]
TAPS = [1, 2, 4, 8, 16, 32]
STRIDE, BLOCKED = 1, 2


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def lp():
    from smfft_amd import large_pfb
    large_pfb.lib()
    before = dict(_worst)
    for k in _worst:
        _worst[k] = 0.0
    yield large_pfb
    print(f"\nworst seen: complex relL2 {_worst['l2']:.3e} (bound {ROW_REL_L2}), max {_worst['max']:.3e} (bound {ROW_MAX}); "
          f"power L1 {_worst['pl1']:.3e} (bound {POWER_L1}), max {_worst['pmax']:.3e} (bound {POWER_MAX})")
    for k in _worst:
        _worst[k] = max(_worst[k], before[k])


def _tuned(lp, schedule, max_workgroups):
    """a launcher for _run: smfft_large_pfb_launch_tuned with this schedule and grid"""
    return lambda *a: lp.launch_tuned(*a[:-1], schedule=schedule, max_workgroups=max_workgroups, power=a[-1])


def _check_both_modes(sm, lp, x, h, N, what, launcher=None):
    ref, s = lpm.pfb(x, h, N), lpm.scale(x, h, N)
    _check_complex(_run(sm, lp, x, h, N, False, launcher=launcher), ref, s, what)
    _check_power(_run(sm, lp, x, h, N, True, launcher=launcher), ref.real ** 2 + ref.imag ** 2, what + " power")


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("P", TAPS)
def test_filter_bank_matches_the_model(sm, lp, P):
    """both lengths x every prototype x (C, F) in {(1, 1), (1, 3), (3, 5)} (one pair; one stream; pairs of three streams on one grid),
    ragged tails, both modes, Gaussian signals"""
    for N in SIZES:
        rng = np.random.default_rng(1000 * N + P)
        protos = {"windowed sinc": lp.prototype(N, P), "gaussian": rng.standard_normal(P * N).astype(np.float32), "ones": np.ones(P * N, np.float32)}
        for C, F, tail in ((1, 1, 0), (1, 3, N - 1), (3, 5, N // 2 + 3)):
            x = _rand(rng, (C, _length(N, P, F, tail)))
            for name, h in protos.items():
                assert lp.frames(x.shape[1], N, P) == F
                _check_both_modes(sm, lp, x, h, N, f"N={N} P={P} {name} C={C} F={F}")


def test_multi_round_through_launch_tuned(sm, lp):
    """74 pairs of two streams on a grid of 16: four rounds and a ragged one of ten, at both lengths under either schedule"""
    P, C, F = 4, 2, 37
    for N in SIZES:
        rng = np.random.default_rng([N, 3])
        x, h = _rand(rng, (C, _length(N, P, F, 100))), rng.standard_normal(P * N).astype(np.float32)
        for schedule in (STRIDE, BLOCKED):
            _check_both_modes(sm, lp, x, h, N, f"N={N} schedule={schedule} grid 16, 74 pairs", launcher=_tuned(lp, schedule, 16))


def test_full_grid(sm, lp):
    """one default launch per length with more pairs than the device's grid: a full round and a ragged one of half the grid and one"""
    from smfft_amd import large
    for N in SIZES:
        grid = large.grid(N)
        rng = np.random.default_rng([N, 5])
        P, F = 4, grid + grid // 2 + 1
        x, h = _rand(rng, (1, _length(N, P, F, 9))), lp.prototype(N, P)
        _check_complex(_run(sm, lp, x, h, N, False), lpm.pfb(x, h, N), lpm.scale(x, h, N), f"N={N} full grid {grid}, {F} pairs")


def test_one_tap_of_ones_is_a_bare_transform(sm, lp):
    """P = 1, h = 1: the library's per-FFT bounds (oracle/np_reference.py)"""
    F = 5
    for N in SIZES:
        rng = np.random.default_rng(N)
        x = _rand(rng, (2, F * N + 5))
        got = _run(sm, lp, x, np.ones(N, np.float32), N, False)
        want = np.fft.fft(x[:, :F * N].astype(np.complex128).reshape(2, F, N), axis=-1)
        l2, mx = assert_close_fp32(got.reshape(-1, N), want.reshape(-1, N), f"large PFB P=1 h=1 N={N}")
        print(f"N={N}: relL2 {l2:.3e} (tol {REL_L2_TOL}) max {mx:.3e} (tol {MAX_ABS_TOL})")


# ------------------------------------------------------------------------------------------------ bit identity
def test_every_schedule_and_grid_gives_the_same_bits(sm, lp):
    """74 pairs: one workgroup; grids of 8, 16 and 24 (multiples of 8); 20 (rounded down to 16 by the blocked schedule); the device's"""
    for N, P, power in ((8192, 8, False), (16384, 4, True)):
        _same_bits_for_every_schedule_and_grid(sm, lp, N, P, power)


def _same_bits_for_every_schedule_and_grid(sm, lp, N, P, power):
    rng = np.random.default_rng(N + P)
    C, F = 2, 37
    x, h = _rand(rng, (C, _length(N, P, F, 9))), lp.prototype(N, P)
    base = _run(sm, lp, x, h, N, power)
    for schedule in (STRIDE, BLOCKED):
        for max_workgroups in (1, 8, 16, 20, 24, 0):
            got = _run(sm, lp, x, h, N, power, launcher=_tuned(lp, schedule, max_workgroups))
            assert np.array_equal(_bits(got), _bits(base)), f"N={N} P={P} schedule={schedule} max_workgroups={max_workgroups}"
    ref = lpm.pfb(x, h, N)
    if power:
        _check_power(base, ref.real ** 2 + ref.imag ** 2, f"schedules N={N}")
    else:
        _check_complex(base, ref, lpm.scale(x, h, N), f"schedules N={N}")


def test_three_streams_equal_three_launches(sm, lp):
    for N, P in ((8192, 4), (16384, 2)):
        rng = np.random.default_rng(N)
        x, h = _rand(rng, (3, _length(N, P, 5, 5))), rng.standard_normal(P * N).astype(np.float32)
        for power in (False, True):
            together = _run(sm, lp, x, h, N, power)
            for c in range(3):
                alone = _run(sm, lp, x[c:c + 1], h, N, power)
                assert np.array_equal(_bits(alone[0]), _bits(together[c])), (N, P, power, c)


# ------------------------------------------------------------------------------------------------ the ABI's corners
def test_caller_stream(sm, lp):
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value
    rng = np.random.default_rng(11)
    N, P, C, F = 8192, 8, 2, 7
    x, h = _rand(rng, (C, _length(N, P, F, 100))), lp.prototype(N, P)

    def on_stream(*a):
        lp.launch(*a[:-1], power=a[-1], stream=stream.value)
        assert hip.hipStreamSynchronize(stream) == 0

    _check_both_modes(sm, lp, x, h, N, "caller's stream", launcher=on_stream)
    assert hip.hipStreamDestroy(stream) == 0


def test_benchmark_adds_to_its_total(sm, lp):
    rng = np.random.default_rng(12)
    N, P, C, F = 16384, 4, 1, 40
    x, h = _rand(rng, (C, _length(N, P, F, 1))), lp.prototype(N, P)
    seen = []

    def timed(*a):
        d_signal, L, C_, d_taps, N_, P_, d_output, power = a
        t = ctypes.c_double(5.0)
        assert lp.lib().smfft_large_pfb_benchmark(d_signal, L, C_, d_taps, N_, P_, int(power), d_output, ctypes.byref(t)) == 0
        first = t.value
        assert first > 5.0
        assert lp.lib().smfft_large_pfb_benchmark(d_signal, L, C_, d_taps, N_, P_, int(power), d_output, ctypes.byref(t)) == 0
        assert t.value > first
        rc, ms = lp.benchmark(d_signal, L, C_, d_taps, N_, P_, d_output, power=power)
        assert rc == 0 and ms > 0.0
        seen.append(ms)

    _check_complex(_run(sm, lp, x, h, N, False, launcher=timed), lpm.pfb(x, h, N), lpm.scale(x, h, N), "benchmark form")
    assert len(seen) == 1


def test_interior_pointers(sm, lp):
    """signal, taps and output at odd element offsets inside their buffers (8-byte aligned, 4 for taps and the power output)"""
    rng = np.random.default_rng(13)
    for N, P in ((8192, 4), (16384, 2)):
        x, h = _rand(rng, (2, _length(N, P, 3, 3))), rng.standard_normal(P * N).astype(np.float32)
        ref = lpm.pfb(x, h, N)
        _check_complex(_run(sm, lp, x, h, N, False, in_off=3, tap_off=1, out_off=5), ref, lpm.scale(x, h, N), f"interior N={N}")
        _check_power(_run(sm, lp, x, h, N, True, in_off=1, tap_off=3, out_off=1), ref.real ** 2 + ref.imag ** 2, f"interior N={N} power")


def test_offsets_beyond_two_to_the_31(sm, lp):
    """N = 16384, P = 4, C = 3, F = 43691: 2^31 + 163855 input elements and 2^31 + 16384 output elements in one launch (17 GiB in, 17 GiB
    out, as in tests/test_pfb_gpu.py's test of this name: the same output size, and 141317 input elements -- 1.1 MB -- more, because a frame
    here is 16384 elements), complex mode.  The signal is made on the device: stream c is an
    uploaded Gaussian block of 2^24 + 1 elements repeated from a stream-dependent phase, x_c[i] = B[(i + 4099 c + 17) mod (2^24 + 1)]
    -- the block length is odd and every sampled window starts at another phase of it, so no two sampled windows are equal.  Sampled
    pairs -- the first, the last, the two either side of output element 2^31 and the two either side of each stream boundary --
    against the model on the input slice copied back."""
    N, P, C = 16384, 4, 3
    F = 43691
    L = _length(N, P, F, 5)
    assert C * L > 1 << 31 and C * F * N > 1 << 31 and C * F * N == (1 << 31) + N
    B = (1 << 24) + 1
    rng = np.random.default_rng(14)
    block = _rand(rng, (B,))
    h = lp.prototype(N, P)
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
    lp.launch(dx.ptr + GUARD * 8, L, C, dh.ptr, N, P, dout.ptr)
    assert sm.lib.smfft_synchronize() == 0
    guard = np.empty(GUARD * 8, np.uint8)
    assert sm.lib.smfft_memcpy_d2h(guard.ctypes.data, dout.ptr + C * F * N * 8, guard.nbytes) == 0
    assert np.all(guard == 0x5A), "the kernel wrote past its output"
    split = (1 << 31) // N                                   # the pair that holds output element 2^31: the last one
    pairs = [0, split - 1, split, F - 1, F, 2 * F - 1, 2 * F]
    assert split == C * F - 1 and 2 * F < split - 1
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
        _check_complex(got, lpm.pfb(xs, h, N), lpm.scale(xs, h, N), f"2^31: pair {g} (c={c}, f={f})")
    for b in (dblock, dh, dx, dout):
        b.free()


# ------------------------------------------------------------------------------------------------ the host conveniences
def test_channelize_and_prototype_on_two_tones(sm, lp):
    """a unit tone at channel 100.37 plus one of a tenth of its amplitude at channel N/2 + 7.5, through prototype() and channelize(): parity
    with the model in both modes (the tones' power bounds of tests/test_pfb_gpu.py), and the leakage of the strong tone alone, from the
    device's power output, against the model's figure for P (tests/test_large_pfb_cpu.py, LEAKAGE).  With E = 2e-6 ||y||_2 sqrt(N) ||s||_2
    the bound on the L1 error of a power row, p the reference power in channel 100 and S the row's total, leakage = (S - p) / p moves
    by at most E / p + S E / p^2 <= 2 E / p (1 + leakage), which is the tolerance; the reference is the model on the same float32
    inputs, itself within 1 % of the figure."""
    from tests.test_large_pfb_cpu import LEAKAGE
    frames = 6
    for N, P in ((N, P) for N in SIZES for P in (2, 8, 32)):
        t = np.arange((frames + P - 1) * N + 13)
        strong = np.exp(2j * np.pi * 100.37 * t / N)
        both = (strong + 0.1 * np.exp(2j * np.pi * (N / 2 + 7.5) * t / N)).astype(np.complex64)
        h = lp.prototype(N, P)
        assert h.dtype == np.float32 and h.shape == (P * N,)
        ref, s = lpm.pfb(both, h, N), lpm.scale(both, h, N)
        got = lp.channelize(both, h, N)
        assert got.shape == ref.shape == (1, frames, N) and got.dtype == np.complex64
        _check_complex(got, ref, s, f"tones N={N} P={P}")
        gotp = lp.channelize(both, h, N, power=True)
        assert gotp.shape == ref.shape and gotp.dtype == np.float32
        refp = ref.real ** 2 + ref.imag ** 2
        d = np.abs(gotp.astype(np.float64) - refp)
        yn, ym, sn = np.linalg.norm(ref, axis=-1), np.abs(ref).max(axis=-1), np.linalg.norm(s, axis=-1)
        l1 = d.sum(axis=-1) / (yn * np.sqrt(N) * sn)
        mx = d.max(axis=-1) / (ym * np.maximum(ym, sn))
        print(f"tones N={N} P={P} power: L1 {l1.max():.3e} max {mx.max():.3e}")
        assert l1.max() <= POWER_L1 and mx.max() <= POWER_MAX, (N, P, l1.max(), mx.max())
        # the strong tone alone
        strong32 = strong.astype(np.complex64)
        refs = lpm.pfb(strong32, h, N)
        refsp = refs.real ** 2 + refs.imag ** 2
        leak_ref = lpm.leakage_of(refsp, 100)
        assert np.all(np.abs(leak_ref - LEAKAGE[P]) <= 0.01 * LEAKAGE[P]), (N, P, leak_ref, LEAKAGE[P])
        leak = lpm.leakage_of(lp.channelize(strong32, h, N, power=True), 100)
        E = POWER_L1 * np.linalg.norm(refs, axis=-1) * np.sqrt(N) * np.linalg.norm(lpm.scale(strong32, h, N), axis=-1)
        tol = 2 * E / refsp[..., 100] * (1 + leak_ref)
        print(f"tones N={N} P={P}: leakage {leak.max():.3g}, model {leak_ref.max():.3g}, figure {LEAKAGE[P]:.3g}, tolerance {tol.max():.3g}")
        assert np.all(np.abs(leak - leak_ref) <= tol), (N, P, leak, leak_ref, tol)

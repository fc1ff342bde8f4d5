"""The bodies of the GPU tests that the channelizer banks share (tests/test_pfb_gpu.py, test_pfb_real_gpu.py and, where its shapes allow,
test_large_pfb_gpu.py), in the manner of tests/addon_checks.py: check_* functions that take the bank (tests/pfb_gpu_harness.py: Bank) and
the shape constants; the modules keep the tests, their parameters, seeds and case tables.  A plain module: no tests, no fixtures."""
import numpy as np

from oracle.np_reference import MAX_ABS_TOL, REL_L2_TOL, assert_close_fp32
from tests import pfb_gpu_harness as gh


def check_filter_bank_matches_the_model(sm, bank, N, P, cases):
    """every prototype x the (C, F, tail) of `cases`, both modes, Gaussian signals"""
    rng = np.random.default_rng(1000 * N + P)
    protos = bank.prototypes(rng, N, P)
    for C, F, tail in cases:
        x = bank.rand(rng, (C, bank.length(N, P, F, tail)))
        for name, h in protos.items():
            ref, s = bank.reference(x, h, N)
            assert ref.shape == (C, F, N + bank.real) and bank.lib.frames(x.shape[1], N, P) == F
            what = f"N={N} P={P} {name} C={C} F={F}"
            bank.check(bank.run(sm, x, h, N, False), ref, s, False, what)
            bank.check(bank.run(sm, x, h, N, True), ref, s, True, what + " power")


def check_one_tap_of_ones_is_a_bare_transform(sm, bank, N, F, tail):
    """P = 1, h = 1 on two streams of F frames: np.fft.fft / rfft of every frame at the library's per-FFT bounds (oracle/np_reference.py)"""
    rng = np.random.default_rng(N)
    W = bank.chunk(N)
    x = bank.rand(rng, (2, F * W + tail))
    got = bank.run(sm, x, np.ones(W, np.float32), N, False)
    frames = x[:, :F * W].astype(np.float64 if bank.real else np.complex128).reshape(2, F, W)
    if bank.real:
        got, want = gh.unpack(got), np.fft.rfft(frames, axis=-1)
    else:
        want = np.fft.fft(frames, axis=-1)
    l2, mx = assert_close_fp32(got.reshape(-1, want.shape[-1]), want.reshape(-1, want.shape[-1]), f"{bank.label} P=1 h=1 N={N}")
    print(f"N={N}: relL2 {l2:.3e} (tol {REL_L2_TOL}) max {mx:.3e} (tol {MAX_ABS_TOL})")


def check_every_schedule_gives_the_same_bits(sm, bank, N, P, power, tiles, tail):
    """one stream of `tiles` tiles less a frame at run lengths 1, 3, 16 and one above the tile count against the shipped one; the first and
    the last eight frames against the model"""
    rng = np.random.default_rng(N + P)
    W = bank.chunk(N)
    F = tiles * (4096 // N) - 1
    x, h = bank.rand(rng, (1, bank.length(N, P, F, tail))), bank.lib.prototype(N, P)
    base = bank.run(sm, x, h, N, power)
    for R in (1, 3, 16, tiles + 7):
        got = bank.run(sm, x, h, N, power, launcher=bank.tuned(R))
        assert np.array_equal(gh.bits(got), gh.bits(base)), f"N={N} P={P} R={R}"
    for f0 in (0, F - 8):
        bank.check_rows(base[:, f0:f0 + 8], x[:, f0 * W:(f0 + 8 + P - 1) * W], h, N, power, f"schedules N={N} frames {f0}...")


def check_three_streams_equal_three_launches(sm, bank, N, P, F, tail):
    rng = np.random.default_rng(N)
    x, h = bank.rand(rng, (3, bank.length(N, P, F, tail))), bank.taps(rng, N, P)
    for power in (False, True):
        together = bank.run(sm, x, h, N, power)
        for c in range(3):
            alone = bank.run(sm, x[c:c + 1], h, N, power)
            assert np.array_equal(gh.bits(alone[0]), gh.bits(together[c])), (N, P, power, c)


def check_caller_stream(sm, bank, N, P, C, F, power_what):
    """power_what: what the power run's line adds to "caller's stream\""""
    rng = np.random.default_rng(11)
    lib = bank.lib
    x, h = bank.rand(rng, (C, bank.length(N, P, F, 100))), lib.prototype(N, P)
    with gh.caller_stream() as (stream, wait):
        def on_stream(*a):
            lib.launch(*a[:-1], power=a[-1], stream=stream)
            wait()
        bank.check_both_modes(sm, x, h, N, "caller's stream", launcher=on_stream, power_what=power_what)


def check_benchmark_adds_to_its_total(sm, bank, N, P, C, F, tail):
    rng = np.random.default_rng(12)
    lib = bank.lib
    x, h = bank.rand(rng, (C, bank.length(N, P, F, tail))), lib.prototype(N, P)
    fn = getattr(lib.lib(), f"smfft_{bank.name}_benchmark")
    seen = []

    def timed(d_signal, L, C_, d_taps, N_, P_, d_output, power):
        gh.benchmark_twice(lambda t: fn(d_signal, L, C_, d_taps, N_, P_, int(power), d_output, t),
                           lambda: lib.benchmark(d_signal, L, C_, d_taps, N_, P_, d_output, power=power), seen)

    bank.check_rows(bank.run(sm, x, h, N, False, launcher=timed), x, h, N, False, "benchmark form")
    assert len(seen) == 1


def check_interior_pointers(sm, bank, shapes, tail, complex_offsets, power_offsets):
    """the three pointers inside their buffers: shapes (N, P, F); the offsets are (in_off, tap_off, out_off) of a complex and a power run"""
    rng = np.random.default_rng(13)
    for N, P, F in shapes:
        x, h = bank.rand(rng, (2, bank.length(N, P, F, tail))), bank.taps(rng, N, P)
        ref, s = bank.reference(x, h, N)
        for power, (in_off, tap_off, out_off) in ((False, complex_offsets), (True, power_offsets)):
            got = bank.run(sm, x, h, N, power, in_off=in_off, tap_off=tap_off, out_off=out_off)
            bank.check(got, ref, s, power, f"interior N={N}" + (" power" if power else ""))


def check_offsets_beyond_two_to_the_31(sm, bank, N, P, C, F, pairs):
    """C streams of F frames and 5 samples more in one launch, complex mode, on the periodic device signal of the harness; the sampled
    `pairs` (c F + f) against the model on the input slice copied back"""
    L = bank.length(N, P, F, 5)
    assert C * L > 1 << 31 and C * F * N > 1 << 31
    lib = bank.lib
    h = lib.prototype(N, P)
    run = gh.PeriodicLaunch(sm, 14, h, C, L, L, C * F, N, np.complex64, lambda dx, dh, dy: lib.launch(dx, L, C, dh, N, P, dy))
    for g in pairs:
        c, f = divmod(g, F)
        bank.check_rows(run.row(g), run.window(c, f * N, P * N), h, N, False, f"2^31: pair {g} (c={c}, f={f})")
    run.free()


def check_two_tones_parity(sm, bank, N, P, both, frames):
    """prototype() and channelize() on the two-tone signal `both` of `frames` frames: shapes, dtypes and parity with the model in every
    output form; -> the prototype"""
    lib = bank.lib
    W = bank.chunk(N)
    h = lib.prototype(N, P)
    assert h.dtype == np.float32 and h.shape == (P * W,)
    ref, s = bank.reference(both, h, N)
    got = lib.channelize(both, h, N)
    assert got.shape == ref.shape == (1, frames, N + bank.real) and got.dtype == np.complex64
    if bank.real:
        packed = lib.channelize(both, h, N, packed=True)
        assert packed.shape == (1, frames, N) and packed.dtype == np.complex64
        assert np.array_equal(gh.bits(lib.unpack(packed)), gh.bits(got)), "channelize unpacks what the device wrote"
        got = packed
    bank.check(got, ref, s, False, f"tones N={N} P={P}")
    gotp = lib.channelize(both, h, N, power=True)
    assert gotp.shape == (1, frames, N) and gotp.dtype == np.float32
    bank.check_tone_power(gotp, ref, s, N, P)
    return h

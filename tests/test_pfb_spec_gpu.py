"""Integrated power spectra of the polyphase filter banks on an MI355X (smfft_pfb_spec_* / smfft_pfb_real_spec_*, smfft_amd.pfb_spec)
against the fp64 model of tools/pfb_spec_model.py: every length, both banks, over taps per channel, prototypes, streams, spectra and
integration lengths; bit identity with the shipped power mode summed in frame order; bit identity across grids and across stream
splits; a caller's stream, the benchmark form, interior pointers, 64-bit offsets.

Every run goes through _run: the output is prefilled with 0xFF (NaN) and followed by a 4096-element guard of 0x5A that must stay
untouched; the signal buffer carries NaN in 4096 samples before stream 0, after stream C - 1, and in every stream's unread tail, which
here starts at (I T + P - 1) frames: the trailing frames f >= I T are not computed, so their samples are not read (the tail belongs to
its own stream, so this never touches another stream's frames).  A read outside the contract shows up as a non-finite output.

Tolerances, per output spectrum (one (c, i) row of N values, S = sum_t p_t).  The shipped power mode holds, per frame,
||got_t - p_t||_1 <= POWER_L1 ||p_t||_1 and max|got_t - p_t| <= POWER_MAX max_k p_t (tests/test_pfb_gpu.py: 2e-6, 1e-5).  Summing T
non-negative fp32 terms sequentially adds, per element, at most gamma sum_t got_t with gamma = (T - 1) u / (1 - (T - 1) u), u = 2^-24
(Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  Hence, with m = sum_t max_k p_t[k] (the model returns it):
    ||got - ref||_1 <= (POWER_L1 + gamma) ||ref||_1      and      max|got - ref| <= (POWER_MAX + gamma) m
(the products of the two small terms are below 1e-11 relative at every T here and are not written out).

The module is ONE test, test_integrated_spectra: the GPU suite already holds five thousand tests, and the library's ten kernels share one
loop, so the lengths, the banks and the cases are loops inside it, in the manner of tests/test_pfb_probes_gpu.py.  Each part is a
check_* function that names its case in every failure message; the probes of tests/test_pfb_spec_probes_gpu.py are its last part.  The
whole takes about three seconds on an MI355X."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import pfb_spec_model as psm  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [256, 512, 1024, 2048, 4096]
BANKS = [False, True]           # real
POWER_L1, POWER_MAX = 2e-6, 1e-5
GUARD = 4096                   # samples around the signal that are NaN, floats after the output that must stay untouched
worst = {"l1": 0.0, "max": 0.0}


def gamma(T):
    u = 2.0 ** -24
    return (T - 1) * u / (1 - (T - 1) * u)


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def ps():
    from smfft_amd import pfb_spec
    pfb_spec.lib()
    yield pfb_spec
    print(f"\nworst seen, relative to its bound: L1 {worst['l1']:.3f}, max {worst['max']:.3f}")


def _name(real):
    return "real" if real else "complex"


def _chunk(N, real):
    """samples of a frame's hop"""
    return 2 * N if real else N


def _rand(rng, shape, real):
    if real:
        return rng.standard_normal(shape).astype(np.float32)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def _length(N, P, frames, tail, real):
    """samples of a stream with `frames` whole frames and `tail` more samples"""
    assert tail < _chunk(N, real) and not (real and tail % 2)
    return (frames + P - 1) * _chunk(N, real) + tail


def _nan(n, real):
    return np.full(n, np.nan, np.float32) if real else np.full(n, np.nan + 1j * np.nan, np.complex64)


def _signal_with_nans(x, N, P, T, real):
    """the device image of x (C, L): NaN in GUARD samples before and after, and in every stream's unread tail"""
    C, L = x.shape
    n = psm.spectra(L, N, P, T, real)
    used = (n * T + P - 1) * _chunk(N, real) if n else 0
    body = x.copy()
    body[:, used:] = np.nan if real else np.nan + 1j * np.nan
    return np.concatenate([_nan(GUARD, real), body.reshape(-1), _nan(GUARD, real)])


def _run(sm, ps, x, h, N, T, real, launcher=None, in_off=0, tap_off=0, out_off=0, finite=True):
    """launch through the device-pointer API (launcher(d_signal, L, C, d_taps, N, P, T, d_output) or ps.launch) from a signal fenced with
    NaN into an output fenced with a guard; returns the (C, I, N) result after checking that the guard is untouched and nothing of the
    prefill is left.  in_off (samples), tap_off and out_off (floats) shift the three pointers into their buffers.  finite=False is for
    runs whose inputs hold NaN on purpose (tests/test_pfb_spec_probes_gpu.py): the guards are checked all the same."""
    C, L = x.shape
    P = h.size // _chunk(N, real)
    n = psm.spectra(L, N, P, T, real)
    sample = 4 if real else 8
    image = _signal_with_nans(x, N, P, T, real)
    if in_off:
        image = np.concatenate([_nan(in_off, real), image])
    dx = sm.DeviceBuffer.from_host(image)
    dh = sm.DeviceBuffer.from_host(np.concatenate([np.full(tap_off, np.nan, np.float32), h]))
    total = C * n * N
    dout = sm.DeviceBuffer((out_off + total + GUARD) * 4)
    if out_off:
        assert sm.lib.smfft_memset(dout.ptr, 0x5A, out_off * 4) == 0
    if total:
        assert sm.lib.smfft_memset(dout.ptr + out_off * 4, 0xFF, total * 4) == 0
    assert sm.lib.smfft_memset(dout.ptr + (out_off + total) * 4, 0x5A, GUARD * 4) == 0
    args = (dx.ptr + (in_off + GUARD) * sample, L, C, dh.ptr + tap_off * 4, N, P, T, dout.ptr + out_off * 4)
    if launcher is None:
        ps.launch(*args, real=real)
    else:
        launcher(*args)
    assert sm.lib.smfft_synchronize() == 0
    raw = dout.to_host(np.uint8, ((out_off + total + GUARD) * 4,))
    assert np.all(raw[:out_off * 4] == 0x5A), "the kernel wrote before its output"
    assert np.all(raw[(out_off + total) * 4:] == 0x5A), "the kernel wrote past its output"
    out = raw[out_off * 4:(out_off + total) * 4].view(np.float32).reshape(C, n, N)
    assert not finite or np.all(np.isfinite(out)), "outputs left unwritten, or a sample read outside the contract"
    for b in (dx, dh, dout):
        b.free()
    return out


def _check(got, ref, m, T, what):
    """got, ref: (C, I, N); m: (C, I)"""
    assert got.shape == ref.shape and got.dtype == np.float32
    d = np.abs(got.astype(np.float64) - ref)
    l1 = d.sum(axis=-1) / ref.sum(axis=-1) / (POWER_L1 + gamma(T))
    mx = d.max(axis=-1) / m / (POWER_MAX + gamma(T))
    print(f"{what}: L1 {l1.max() * (POWER_L1 + gamma(T)):.3e} (bound {POWER_L1 + gamma(T):.3e}) max {mx.max() * (POWER_MAX + gamma(T)):.3e} "
          f"(bound {POWER_MAX + gamma(T):.3e})")
    worst["l1"], worst["max"] = max(worst["l1"], l1.max()), max(worst["max"], mx.max())
    assert l1.max() <= 1.0 and mx.max() <= 1.0, f"{what}: L1 {l1.max():.3f} max {mx.max():.3f} of their bounds"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ parity
def check_integrated_spectra_match_the_model(sm, ps, N, real):
    """P in {1, 3, 32} x windowed-sinc and Gaussian prototypes x (C, I, T, extra frames) in {(1, 1, 1, 0), (1, per + 1, 3, 2),
    (3, 2 per + 1, 2, 1), (2, 3 per, 17, 0)}, per = 4096 / N (one group; a partial second tile and frames left over; tiles straddling
    streams; whole tiles and a long sum), ragged tails, Gaussian signals"""
    rng = np.random.default_rng(10 * N + real)
    per = 4096 // N
    for P in (1, 3, 32):
        protos = {"windowed sinc": ps.prototype(N, P, real=real), "gaussian": rng.standard_normal(P * _chunk(N, real)).astype(np.float32)}
        for C, n, T, extra in ((1, 1, 1, 0), (1, per + 1, 3, 2), (3, 2 * per + 1, 2, 1), (2, 3 * per, 17, 0)):
            L = _length(N, P, n * T + extra, 2 * (N // 4 + 3), real)
            x = _rand(rng, (C, L), real)
            assert ps.spectra(L, N, P, T, real=real) == n and extra < T
            for name, h in protos.items():
                ref, m = psm.integrate(x, h, N, T, real)
                _check(_run(sm, ps, x, h, N, T, real), ref, m, T, f"{_name(real)} N={N} P={P} {name} C={C} I={n} T={T}")


# ------------------------------------------------------------------------------------------------ bit identity
def _power_mode(sm, x, h, N, real):
    """(C, F, N) float32: what the shipped bank's power mode writes for x"""
    from smfft_amd import pfb, pfb_real
    bank = pfb_real if real else pfb
    C, L = x.shape
    P = h.size // _chunk(N, real)
    F = bank.frames(L, N, P)
    dx, dh = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer.from_host(h)
    dout = sm.DeviceBuffer(C * F * N * 4)
    assert sm.lib.smfft_memset(dout.ptr, 0xFF, dout.nbytes) == 0
    bank.launch(dx.ptr, L, C, dh.ptr, N, P, dout.ptr, power=True)
    assert sm.lib.smfft_synchronize() == 0
    out = dout.to_host(np.float32, (C, F, N))
    for b in (dx, dh, dout):
        b.free()
    assert np.all(np.isfinite(out))
    return out


def _sequential_sum(p, n, T):
    """(C, F, N) float32 -> (C, n, N): acc = p_0, acc = acc + p_t, in fp32 in frame order"""
    p = p[:, :n * T].reshape(p.shape[0], n, T, p.shape[-1])
    acc = p[:, :, 0].copy()
    for t in range(1, T):
        acc = acc + p[:, :, t]
    assert acc.dtype == np.float32
    return acc


def check_output_is_the_shipped_power_mode_summed_in_frame_order(sm, ps, N, real):
    """T in {1, 2, 5}: the output equals, bit for bit, the fp32 sequential sum of what the bank's own power=1 launch writes for the same
    signal and taps; T = 1 is the power mode itself.  The definition -- and what a re-fused accumulation breaks."""
    rng = np.random.default_rng(20 * N + real)
    per = 4096 // N
    P, C = 4, 2
    h = ps.prototype(N, P, real=real)
    x = _rand(rng, (C, _length(N, P, 5 * (per + 1) + 1, 6, real)), real)
    p = _power_mode(sm, x, h, N, real)
    for T in (1, 2, 5):
        n = ps.spectra(x.shape[1], N, P, T, real=real)
        assert n == (5 * (per + 1) + 1) // T
        got = _run(sm, ps, x, h, N, T, real)
        assert np.array_equal(_bits(got), _bits(_sequential_sum(p, n, T))), f"{_name(real)} N={N} T={T}"


def check_every_grid_gives_the_same_bits(sm, ps, N, real):
    """5 per + 1 groups = five whole tiles and a partial one: grids of 1, 2 and 7 workgroups (every tile in one loop; three rounds; more
    workgroups than tiles) against the shipped grid"""
    rng = np.random.default_rng(30 * N + real)
    per = 4096 // N
    P, T = 2, 3
    x, h = _rand(rng, (1, _length(N, P, (5 * per + 1) * T + 1, 0, real)), real), rng.standard_normal(P * _chunk(N, real)).astype(np.float32)
    base = _run(sm, ps, x, h, N, T, real)
    assert base.shape == (1, 5 * per + 1, N)
    for G in (1, 2, 7):
        got = _run(sm, ps, x, h, N, T, real, launcher=lambda *a, G=G: ps.launch_tuned(*a, G, real=real))
        assert np.array_equal(_bits(got), _bits(base)), f"{_name(real)} N={N} G={G}"
    ref, m = psm.integrate(x, h, N, T, real)
    _check(base, ref, m, T, f"grids {_name(real)} N={N}")


def check_three_streams_equal_three_launches(sm, ps, N, real):
    rng = np.random.default_rng(40 * N + real)
    P, T = 4, 3
    n = 2 * (4096 // N) + 1                       # tiles straddle the streams
    x, h = _rand(rng, (3, _length(N, P, n * T + 2, 10, real)), real), rng.standard_normal(P * _chunk(N, real)).astype(np.float32)
    together = _run(sm, ps, x, h, N, T, real)
    assert together.shape == (3, n, N)
    for c in range(3):
        alone = _run(sm, ps, x[c:c + 1], h, N, T, real)
        assert np.array_equal(_bits(alone[0]), _bits(together[c])), (N, real, c)


# ------------------------------------------------------------------------------------------------ the ABI's corners
def check_caller_stream(sm, ps, real):
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value
    rng = np.random.default_rng(51 + real)
    N, P, C, T = 1024, 8, 2, 4
    x, h = _rand(rng, (C, _length(N, P, 9 * T + 3, 100, real)), real), ps.prototype(N, P, real=real)

    def on_stream(*a):
        ps.launch(*a, real=real, stream=stream.value)
        assert hip.hipStreamSynchronize(stream) == 0

    ref, m = psm.integrate(x, h, N, T, real)
    _check(_run(sm, ps, x, h, N, T, real, launcher=on_stream), ref, m, T, f"caller's stream, {_name(real)}")
    assert hip.hipStreamDestroy(stream) == 0


def check_benchmark_adds_to_its_total(sm, ps, real):
    rng = np.random.default_rng(52 + real)
    N, P, C, T = 2048, 4, 1, 8
    x, h = _rand(rng, (C, _length(N, P, 40 * T, 2, real)), real), ps.prototype(N, P, real=real)
    fn = getattr(ps.lib(), ps.PREFIXES[real] + "_benchmark")
    seen = []

    def timed(*a):
        t = ctypes.c_double(5.0)
        assert fn(*a, ctypes.byref(t)) == 0
        first = t.value
        assert first > 5.0
        assert fn(*a, ctypes.byref(t)) == 0
        assert t.value > first
        rc, ms = ps.benchmark(*a, real=real)
        assert rc == 0 and ms > 0.0
        seen.append(ms)

    ref, m = psm.integrate(x, h, N, T, real)
    _check(_run(sm, ps, x, h, N, T, real, launcher=timed), ref, m, T, f"benchmark form, {_name(real)}")
    assert len(seen) == 1


def check_interior_pointers(sm, ps, real):
    """signal, taps and output at odd element offsets inside their buffers: an odd number of float2 for the signal (and for the real
    bank's coefficient pairs), an odd number of floats for the complex bank's taps and for the output"""
    rng = np.random.default_rng(53 + real)
    for N, P, T in ((256, 4, 3), (4096, 2, 2)):
        x = _rand(rng, (2, _length(N, P, (4096 // N + 2) * T + 1, 6, real)), real)
        h = rng.standard_normal(P * _chunk(N, real)).astype(np.float32)
        ref, m = psm.integrate(x, h, N, T, real)
        got = _run(sm, ps, x, h, N, T, real, in_off=6 if real else 3, tap_off=2 if real else 1, out_off=5)
        _check(got, ref, m, T, f"interior {_name(real)} N={N}")


def check_offsets_beyond_two_to_the_31(sm, ps):
    """N = 1024, P = 4, T = 64, C = 2, F = 2^20 + 104: 2^31 + 219146 signal elements in one launch of the complex bank (17 GiB in; the
    output is 2 x 16385 spectra, 128 MiB).  The signal is made on the device: stream c is an uploaded Gaussian block of 2^24 + 1
    elements repeated from a stream-dependent phase, x_c[i] = B[(i + 4099 c + 17) mod (2^24 + 1)] -- the block length is odd and every
    sampled window starts at another phase of it.  Sampled spectra -- the first, the last, and the two either side of the stream
    boundary; the last one's window starts beyond element 2^31 -- against the model on the input slice copied back."""
    N, P, C, T = 1024, 4, 2, 64
    F = (1 << 20) + 104
    L = _length(N, P, F, 5, False)
    n = F // T
    assert C * L > 1 << 31 and L + (n - 1) * T * N > 1 << 31 and ps.spectra(L, N, P, T) == n == 16385
    B = (1 << 24) + 1
    rng = np.random.default_rng(54)
    block = _rand(rng, (B,), False)
    h = ps.prototype(N, P)
    dblock, dh = sm.DeviceBuffer.from_host(block), sm.DeviceBuffer.from_host(h)
    dx = sm.DeviceBuffer((C * L + 2 * GUARD) * 8)
    dout = sm.DeviceBuffer((C * n * N + GUARD) * 4)
    assert sm.lib.smfft_memset(dx.ptr, 0xFF, dx.nbytes) == 0
    used = (n * T + P - 1) * N                           # the rest of a stream stays NaN: it is not read
    for c in range(C):
        i, phase = 0, (4099 * c + 17) % B
        while i < used:
            k = min(B - phase, used - i)
            assert sm.lib.smfft_memcpy_d2d(dx.ptr + (GUARD + c * L + i) * 8, dblock.ptr + phase * 8, k * 8) == 0
            i, phase = i + k, 0
    assert sm.lib.smfft_memset(dout.ptr, 0xFF, C * n * N * 4) == 0
    assert sm.lib.smfft_memset(dout.ptr + C * n * N * 4, 0x5A, GUARD * 4) == 0
    ps.launch(dx.ptr + GUARD * 8, L, C, dh.ptr, N, P, T, dout.ptr)
    assert sm.lib.smfft_synchronize() == 0
    guard = np.empty(GUARD * 4, np.uint8)
    assert sm.lib.smfft_memcpy_d2h(guard.ctypes.data, dout.ptr + C * n * N * 4, guard.nbytes) == 0
    assert np.all(guard == 0x5A), "the kernel wrote past its output"
    seen = set()
    for g in (0, C * n - 1, n - 1, n):
        c, i = divmod(g, n)
        xs = np.empty((1, (T + P - 1) * N), np.complex64)
        assert sm.lib.smfft_memcpy_d2h(xs.ctypes.data, dx.ptr + (GUARD + c * L + i * T * N) * 8, xs.nbytes) == 0
        phase = (i * T * N + 4099 * c + 17) % B
        assert np.array_equal(xs[0], np.take(block, np.arange(phase, phase + xs.shape[1]), mode="wrap")) and phase not in seen
        seen.add(phase)
        got = np.empty((1, 1, N), np.float32)
        assert sm.lib.smfft_memcpy_d2h(got.ctypes.data, dout.ptr + g * N * 4, got.nbytes) == 0
        assert np.all(np.isfinite(got))
        ref, m = psm.integrate(xs, h, N, T)
        _check(got, ref, m, T, f"2^31: group {g} (c={c}, i={i})")
    for b in (dblock, dh, dx, dout):
        b.free()


# ------------------------------------------------------------------------------------------------ the one test
def test_integrated_spectra(sm, ps):
    """every check of this module and every probe of tests/test_pfb_spec_probes_gpu.py, at every length in both banks"""
    from tests import test_pfb_spec_probes_gpu as probes
    for real in BANKS:
        for N in SIZES:
            check_integrated_spectra_match_the_model(sm, ps, N, real)
            check_output_is_the_shipped_power_mode_summed_in_frame_order(sm, ps, N, real)
            check_every_grid_gives_the_same_bits(sm, ps, N, real)
        for N in (512, 2048):
            check_three_streams_equal_three_launches(sm, ps, N, real)
        check_caller_stream(sm, ps, real)
        check_benchmark_adds_to_its_total(sm, ps, real)
        check_interior_pointers(sm, ps, real)
    check_offsets_beyond_two_to_the_31(sm, ps)
    for real in BANKS:
        for N in SIZES:
            for probe in probes.PROBES:
                probe(sm, ps, N, real)

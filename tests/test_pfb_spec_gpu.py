"""Integrated power spectra of the polyphase filter banks on an MI355X (smfft_pfb_spec_* / smfft_pfb_real_spec_*, smfft_amd.pfb_spec)
against the fp64 model of tools/pfb_spec_model.py: every length, both banks, over taps per channel, prototypes, streams, spectra and
integration lengths; bit identity with the shipped power mode summed in frame order; bit identity across grids and across stream
splits; a caller's stream, the benchmark form, interior pointers, 64-bit offsets.

Every run goes through the guarded run of tests/pfb_gpu_harness.py (Spectra.run): the output is prefilled with 0xFF (NaN) and followed by a
4096-element guard of 0x5A that must stay untouched; the signal buffer carries NaN in 4096 samples before stream 0, after stream C - 1,
and in every stream's unread tail, which here starts at (I T + P - 1) frames: the trailing frames f >= I T are not computed, so their
samples are not read (the tail belongs to its own stream, so this never touches another stream's frames).  A read outside the contract
shows up as a non-finite output.

Tolerances, per output spectrum (one (c, i) row of N values, S = sum_t p_t).  The shipped power mode holds, per frame,
||got_t - p_t||_1 <= POWER_L1 ||p_t||_1 and max|got_t - p_t| <= POWER_MAX max_k p_t (tests/pfb_gpu_harness.py: 2e-6, 1e-5).  Summing T
non-negative fp32 terms sequentially adds, per element, at most gamma sum_t got_t with gamma = (T - 1) u / (1 - (T - 1) u), u = 2^-24
(Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  Hence, with m = sum_t max_k p_t[k] (the model returns it):
    ||got - ref||_1 <= (POWER_L1 + gamma) ||ref||_1      and      max|got - ref| <= (POWER_MAX + gamma) m
(the products of the two small terms are below 1e-11 relative at every T here and are not written out).

The module is ONE test, test_integrated_spectra: the GPU suite already holds five thousand tests, and the library's ten kernels share one
loop, so the lengths, the banks and the cases are loops inside it, in the manner of tests/test_pfb_probes_gpu.py.  Each part is a
check_* function that names its case in every failure message; the probes of tests/pfb_spec_probes.py are its last part.  The
whole takes about three seconds on an MI355X."""
import numpy as np
import pytest

from tests import pfb_gpu_harness as gh
from tests import pfb_spec_probes as probes
from tests.pfb_gpu_harness import bits as _bits, chunk as _chunk, length as _length, rand as _rand

pytestmark = pytest.mark.gpu

SIZES = gh.SIZES
BANKS = [False, True]           # real


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def ps():
    from smfft_amd import pfb_spec
    pfb_spec.lib()
    spectra = gh.Spectra(pfb_spec)
    yield spectra
    print(f"\nworst seen, relative to its bound: L1 {spectra.worst.get('l1', 0.0):.3f}, max {spectra.worst.get('max', 0.0):.3f}")


def _name(real):
    return "real" if real else "complex"


# ------------------------------------------------------------------------------------------------ parity
def check_integrated_spectra_match_the_model(sm, spec, N, real):
    """P in {1, 3, 32} x windowed-sinc and Gaussian prototypes x (C, I, T, extra frames) in {(1, 1, 1, 0), (1, per + 1, 3, 2),
    (3, 2 per + 1, 2, 1), (2, 3 per, 17, 0)}, per = 4096 / N (one group; a partial second tile and frames left over; tiles straddling
    streams; whole tiles and a long sum), ragged tails, Gaussian signals"""
    rng = np.random.default_rng(10 * N + real)
    per = 4096 // N
    for P in (1, 3, 32):
        protos = {"windowed sinc": spec.ps.prototype(N, P, real=real), "gaussian": rng.standard_normal(P * _chunk(N, real)).astype(np.float32)}
        for C, n, T, extra in ((1, 1, 1, 0), (1, per + 1, 3, 2), (3, 2 * per + 1, 2, 1), (2, 3 * per, 17, 0)):
            L = _length(N, P, n * T + extra, 2 * (N // 4 + 3), real)
            x = _rand(rng, (C, L), real)
            assert spec.ps.spectra(L, N, P, T, real=real) == n and extra < T
            for name, h in protos.items():
                spec.check(spec.run(sm, x, h, N, T, real), x, h, N, T, real, f"{_name(real)} N={N} P={P} {name} C={C} I={n} T={T}")


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


def check_output_is_the_shipped_power_mode_summed_in_frame_order(sm, spec, N, real):
    """T in {1, 2, 5}: the output equals, bit for bit, the fp32 sequential sum of what the bank's own power=1 launch writes for the same
    signal and taps; T = 1 is the power mode itself.  The definition -- and what a re-fused accumulation breaks."""
    rng = np.random.default_rng(20 * N + real)
    per = 4096 // N
    P, C = 4, 2
    h = spec.ps.prototype(N, P, real=real)
    x = _rand(rng, (C, _length(N, P, 5 * (per + 1) + 1, 6, real)), real)
    p = _power_mode(sm, x, h, N, real)
    for T in (1, 2, 5):
        n = spec.ps.spectra(x.shape[1], N, P, T, real=real)
        assert n == (5 * (per + 1) + 1) // T
        got = spec.run(sm, x, h, N, T, real)
        assert np.array_equal(_bits(got), _bits(_sequential_sum(p, n, T))), f"{_name(real)} N={N} T={T}"


def check_every_grid_gives_the_same_bits(sm, spec, N, real):
    """5 per + 1 groups = five whole tiles and a partial one: grids of 1, 2 and 7 workgroups (every tile in one loop; three rounds; more
    workgroups than tiles) against the shipped grid"""
    rng = np.random.default_rng(30 * N + real)
    per = 4096 // N
    P, T = 2, 3
    x, h = _rand(rng, (1, _length(N, P, (5 * per + 1) * T + 1, 0, real)), real), rng.standard_normal(P * _chunk(N, real)).astype(np.float32)
    base = spec.run(sm, x, h, N, T, real)
    assert base.shape == (1, 5 * per + 1, N)
    for G in (1, 2, 7):
        got = spec.run(sm, x, h, N, T, real, launcher=lambda *a, G=G: spec.ps.launch_tuned(*a, G, real=real))
        assert np.array_equal(_bits(got), _bits(base)), f"{_name(real)} N={N} G={G}"
    spec.check(base, x, h, N, T, real, f"grids {_name(real)} N={N}")


def check_three_streams_equal_three_launches(sm, spec, N, real):
    rng = np.random.default_rng(40 * N + real)
    P, T = 4, 3
    n = 2 * (4096 // N) + 1                       # tiles straddle the streams
    x, h = _rand(rng, (3, _length(N, P, n * T + 2, 10, real)), real), rng.standard_normal(P * _chunk(N, real)).astype(np.float32)
    together = spec.run(sm, x, h, N, T, real)
    assert together.shape == (3, n, N)
    for c in range(3):
        alone = spec.run(sm, x[c:c + 1], h, N, T, real)
        assert np.array_equal(_bits(alone[0]), _bits(together[c])), (N, real, c)


# ------------------------------------------------------------------------------------------------ the ABI's corners
def check_caller_stream(sm, spec, real):
    rng = np.random.default_rng(51 + real)
    N, P, C, T = 1024, 8, 2, 4
    x, h = _rand(rng, (C, _length(N, P, 9 * T + 3, 100, real)), real), spec.ps.prototype(N, P, real=real)
    with gh.caller_stream() as (stream, wait):
        def on_stream(*a):
            spec.ps.launch(*a, real=real, stream=stream)
            wait()
        spec.check(spec.run(sm, x, h, N, T, real, launcher=on_stream), x, h, N, T, real, f"caller's stream, {_name(real)}")


def check_benchmark_adds_to_its_total(sm, spec, real):
    rng = np.random.default_rng(52 + real)
    N, P, C, T = 2048, 4, 1, 8
    x, h = _rand(rng, (C, _length(N, P, 40 * T, 2, real)), real), spec.ps.prototype(N, P, real=real)
    fn = getattr(spec.ps.lib(), spec.ps.PREFIXES[real] + "_benchmark")
    seen = []

    def timed(*a):
        gh.benchmark_twice(lambda t: fn(*a, t), lambda: spec.ps.benchmark(*a, real=real), seen)

    spec.check(spec.run(sm, x, h, N, T, real, launcher=timed), x, h, N, T, real, f"benchmark form, {_name(real)}")
    assert len(seen) == 1


def check_interior_pointers(sm, spec, real):
    """signal, taps and output at odd element offsets inside their buffers: an odd number of float2 for the signal (and for the real
    bank's coefficient pairs), an odd number of floats for the complex bank's taps and for the output"""
    rng = np.random.default_rng(53 + real)
    for N, P, T in ((256, 4, 3), (4096, 2, 2)):
        x = _rand(rng, (2, _length(N, P, (4096 // N + 2) * T + 1, 6, real)), real)
        h = rng.standard_normal(P * _chunk(N, real)).astype(np.float32)
        got = spec.run(sm, x, h, N, T, real, in_off=6 if real else 3, tap_off=2 if real else 1, out_off=5)
        spec.check(got, x, h, N, T, real, f"interior {_name(real)} N={N}")


def check_offsets_beyond_two_to_the_31(sm, spec):
    """N = 1024, P = 4, T = 64, C = 2, F = 2^20 + 104: 2^31 + 219146 signal elements in one launch of the complex bank (17 GiB in; the
    output is 2 x 16385 spectra, 128 MiB), on the periodic device signal of tests/pfb_gpu_harness.py (PeriodicLaunch); the rest of a
    stream, which is not read, stays NaN.  Sampled spectra -- the first, the last, and the two either side of the stream
    boundary; the last one's window starts beyond element 2^31 -- against the model on the input slice copied back."""
    N, P, C, T = 1024, 4, 2, 64
    F = (1 << 20) + 104
    L = _length(N, P, F, 5, False)
    n = F // T
    assert C * L > 1 << 31 and L + (n - 1) * T * N > 1 << 31 and spec.ps.spectra(L, N, P, T) == n == 16385
    h = spec.ps.prototype(N, P)
    run = gh.PeriodicLaunch(sm, 54, h, C, L, (n * T + P - 1) * N, C * n, N, np.float32, lambda dx, dh, dy: spec.ps.launch(dx, L, C, dh, N, P, T, dy))
    for g in (0, C * n - 1, n - 1, n):
        c, i = divmod(g, n)
        spec.check(run.row(g), run.window(c, i * T * N, (T + P - 1) * N), h, N, T, False, f"2^31: group {g} (c={c}, i={i})")
    run.free()


# ------------------------------------------------------------------------------------------------ the one test
def test_integrated_spectra(sm, ps):
    """every check of this module and every probe of tests/pfb_spec_probes.py, at every length in both banks"""
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

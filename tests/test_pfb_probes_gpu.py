"""The two polyphase filter banks (libsmfft_pfb.so, libsmfft_pfb_real.so) per output element and in isolation, on an MI355X: the twenty
kernels of tests/pfb_inventory.py through one set of tests, parametrized by bank.  Every run goes through the guarded run of
tests/pfb_gpu_harness.py (Bank.run: a NaN-fenced signal into a prefilled, guarded output).
A test is one bank (the probe: one bank and length); its shapes, modes and cases are loops inside it, every failure message names its own,
so that the module adds eighteen tests to the GPU suite, not ninety.

A1  Tap-matrix probe (test_tap_matrix_probe, cases and closed form: tests/pfb_probe_cases.py).  Every frame of the stream sees exactly
    one nonzero sample, a 1.0 at position n of branch p, so the weighted sum is exact and the transform's input is h[p W + n] delta_n:
    the output must be h W_W^{n k}, every (p, position) once, every tap with a value of its own.  Per element, relative to |h| of the
    frame, the error must stay below the transform probes' ceiling (tests/probe_cases.py: probe_ceiling(N, 1) for the complex bank,
    probe_ceiling(2N, 1) for the real one); the two components of the real bank's element 0 are held separately to h and h (-1)^m.
    Power mode: |got - h^2| <= (2 c + 2^-22) h^2 with c that ceiling (| |y + d|^2 - |y|^2 | <= 2 |y| |d| + |d|^2, plus the two roundings
    of fma(x, x, y y)); the real bank's element 0 is h^2, the power of DC alone.  The expected rows are computed in slices of frames.
A2  Ratchet: tests/pfb_accuracy_ratchet.json holds, per case id, the largest and the rms of A1's per-element figures as measured on
    an MI355X (tools/accuracy_ratchet.py --pfb writes it).  The kernels are deterministic, so only a change of a kernel or of the
    compiler moves them; a figure above 1.25 x its entry fails, and so does a case without an entry.
B1  Frames are independent of where they are computed (test_equal_windows_give_equal_bits).  Three streams hold the same Gaussian
    sequence with a period of three chunks, so frame f depends only on f mod 3; at least 2000 tiles (more than two rounds of the
    persistent grid at run length 1) and, where a tile holds more than one frame, a ragged last tile.  Within one launch every frame
    of a class must equal the class's first frame to the bit, in every stream, at run lengths 1 and 4, and the three representatives
    meet the fp64 model under the bank's own row checks.  Consecutive tiles of a workgroup hold different classes in the same LDS
    region, so a missing barrier between tiles changes bits instead of re-reading equal values.
    (What it did not catch on an MI355X: a build without the fft_sync before eng.transform, at any of these lengths, in either bank.
    Between a tile's last LDS read and the next tile's first LDS write every wave runs the stores and the whole tap loop, P rounds of
    thirty-two global loads, and the waves left the transform's own barriers together: the race needs one wave a tap loop ahead of
    another, which these runs never produced.  The barrier stays; this test does not prove it.)
B2  Exact homogeneity (test_streams_and_taps_scale_exactly): stream c scaled by 2^e_c and the taps by 2^g scale the output by
    2^(e_c + g) to the bit (the power by its square, at half the exponents), with tiles straddling the streams.
B3  Non-finite values reach exactly their frames (test_nan_sample_reaches_exactly_its_frames, test_nan_tap_reaches_every_frame): a NaN
    or a +Inf at one sample of chunk j of stream c makes every element of frames max(0, j - P + 1) ... min(j, F - 1) of that stream
    non-finite and leaves every other output word as the clean run wrote it -- the first chunk, the last chunk of the first window, an
    interior one and the last chunk a stream reads (the next stream's frame 0 stays clean; in the last stream the clamped slots of the
    ragged last tile load the poisoned pair again and must store nothing: the guard of the run); a NaN tap makes every element of every
    frame non-finite.  NaN is data here: nothing faults."""
import json
import os

import numpy as np
import pytest

from tests import pfb_gpu_harness as gh
from tests import pfb_probe_cases as ppc
from tests import probe_cases as pc
from tests.pfb_gpu_harness import bits as _bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATCHET = os.path.join(ROOT, "tests", "pfb_accuracy_ratchet.json")
SLICE = 1 << 22                # output elements per slice of A1's expected rows (64 MiB of complex128)
STREAM_SCALES = (-40, -13, 11, 40)
TAP_SCALES = (-7, 5)

BANKS = {name: gh.Bank(name) for name in ("pfb", "pfb_real")}
pm = BANKS["pfb"].model


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    assert smfft_amd.lib.smfft_device_count() >= 1, "no HIP device"
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module", params=sorted(BANKS))
def bank(request):
    return BANKS[request.param]


@pytest.fixture(scope="module")
def ratchet():
    with open(RATCHET) as f:
        return json.load(f)


def _non_finite(out):
    """per output element: a non-finite component"""
    if np.iscomplexobj(out):
        return ~(np.isfinite(out.real) & np.isfinite(out.imag))
    return ~np.isfinite(out)


# ---------------------------------------------------------------------------------------------------- A1 / A2
def probe_errors(sm, case):
    """(largest, rms) of the tap-matrix probe's per-element errors, relative to |h| of the frame (h^2 in power mode); the real bank's
    element 0 counts with the larger of its two components' errors"""
    x, h, pos = ppc.inputs(case)
    got = BANKS[case.bank].run(sm, x, h, case.n, bool(case.power))[0]
    F, N = case.frames, case.n
    assert got.shape == (F, N)
    worst, sq = 0.0, 0.0
    step = max(1, SLICE // N)
    for f0 in range(0, F, step):
        f = np.arange(f0, min(F, f0 + step))
        g = got[f0:f0 + step]
        n, hf = ppc.frame_taps(case, h, pos, f)
        assert np.all(np.abs(hf) >= 0.5)
        if case.power:
            err = np.abs(g.astype(np.float64) - (hf * hf)[:, None]) / (hf * hf)[:, None]
        else:
            want = ppc.expected(case, h, pos, f)
            err = np.abs(g - want[:, :N])
            if case.real:           # element 0 = (X[0], X[N]) = (h, h (-1)^m), each on its own
                err[:, 0] = np.maximum(np.abs(g[:, 0].real - hf), np.abs(g[:, 0].imag - hf * (1 - 2 * (n & 1))))
            err /= np.abs(hf)[:, None]
        worst = max(worst, float(err.max()))
        sq += float(np.sum(err * err))
    return worst, float(np.sqrt(sq / (F * N)))


def _ratchet_failures(ratchet, case, per_elem, rms):
    if case.id not in ratchet:
        return [f"{case.id}: no entry in tests/pfb_accuracy_ratchet.json (tools/accuracy_ratchet.py --pfb measures it)"]
    return [f"{case.id}: {key} = {value:.3e} above {pc.RATCHET_SLACK} x the committed {ratchet[case.id][key]:.3e}"
            for key, value in (("probe_max", per_elem), ("probe_rms", rms)) if value > pc.RATCHET_SLACK * ratchet[case.id][key]]


@pytest.mark.parametrize("N", ppc.SIZES)
def test_tap_matrix_probe(sm, ratchet, bank, N):
    """every case of tests/pfb_probe_cases.py at this bank and length, each held to its ceiling and to its ratchet entry; all of them
    run and print their figures before the test fails on any"""
    cases = [c for c in ppc.CASES if c.bank == bank.name and c.n == N]
    assert {c.power for c in cases} == {0, 1} and {c.tag for c in cases} == {"all", "sub"}
    failures = []
    for case in cases:
        per_elem, rms = probe_errors(sm, case)
        print(f"{case.id}: per element {per_elem:.3e} (ceiling {case.ceiling:.3e}) rms {rms:.3e}")
        if not per_elem <= case.ceiling:
            failures.append(f"{case.id}: per-element error {per_elem:.3e} above the ceiling {case.ceiling:.3e}")
        failures += _ratchet_failures(ratchet, case, per_elem, rms)
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------------- B1
EQUAL_SHAPES = [(256, 4), (1024, 8), (2048, 3), (4096, 2)]
MODES = (False, True)          # complex, power


def test_equal_windows_give_equal_bits(sm, bank):
    for N, P in EQUAL_SHAPES:
        for power in MODES:
            _equal_windows(sm, bank, N, P, power)


def _equal_windows(sm, bank, N, P, power):
    C, Q = 3, 3
    W, per = bank.chunk(N), 4096 // N
    F = -(-2000 * per // C)
    while per > 1 and C * F % per == 0:
        F += 1
    plan = pm.Plan((F + P - 1) * N, N, P, C)         # in float2 units for the real bank: its chunk is N pairs
    assert plan.frames() == F and plan.tiles() >= 2000 and (per == 1 or plan.pair_of(plan.tiles() - 1, per - 1) == -1)
    rng = np.random.default_rng([N, P, bank.real])
    period = bank.rand(rng, (Q * W,))
    chunks = F + P - 1
    stream = np.concatenate([np.tile(period, -(-chunks // Q))[:chunks * W], bank.rand(rng, (6,))])      # + an unread tail
    x, h = np.tile(stream, (C, 1)), bank.taps(rng, N, P)
    for R in (1, 4):
        out = bank.run(sm, x, h, N, power, launcher=bank.tuned(R))
        assert out.shape == (C, F, N)
        bits = _bits(out).reshape(C, F, -1)
        for cls in range(Q):
            same = np.all(bits[:, cls::Q] == bits[0, cls], axis=-1)
            assert same.all(), f"{bank.name} N={N} P={P} power={power} R={R}: frames (stream, index) {np.argwhere(~same)[:8].tolist()} of class {cls} differ from frame {cls}"
        bank.check_rows(out[:1, :Q], x[:1, :(Q + P - 1) * W], h, N, power, f"{bank.name} equal windows N={N} P={P} power={power} R={R}")


# ---------------------------------------------------------------------------------------------------- B2
def test_streams_and_taps_scale_exactly(sm, bank):
    for N, P in [(256, 32), (512, 4), (4096, 4)]:
        for power in MODES:
            _scale_exactly(sm, bank, N, P, power)


def _scale_exactly(sm, bank, N, P, power):
    C = len(STREAM_SCALES)
    W, per = bank.chunk(N), 4096 // N
    F = 2 * per + 1                                    # tiles straddle the streams
    rng = np.random.default_rng([N, P, bank.real, 2])
    x, h = bank.rand(rng, (C, (F + P - 1) * W + 6)), bank.taps(rng, N, P)
    clean = bank.run(sm, x, h, N, power)
    # power mode: half the exponents, so that the doubled sum stays within +-80
    e = np.array([int(s / 2) for s in STREAM_SCALES] if power else STREAM_SCALES)
    for g in TAP_SCALES:
        g = int(g / 2) if power else g
        got = bank.run(sm, x * np.float32(2.0) ** e[:, None].astype(np.float32), h * np.float32(2.0 ** g), N, power)
        k = 2 if power else 1
        want = np.ldexp(clean.view(np.float32).reshape(C, F, -1), (k * (e + g))[:, None, None])
        assert np.all(np.isfinite(want)) and np.all((want != 0) == (clean.view(np.float32).reshape(C, F, -1) != 0))
        same = np.all(_bits(got).reshape(C, F, -1) == _bits(want), axis=-1)
        assert same.all(), f"{bank.name} N={N} P={P} power={power} taps 2^{g}: frames (stream, index) {np.argwhere(~same)[:8].tolist()} do not scale exactly"


# ---------------------------------------------------------------------------------------------------- B3
NAN_SHAPES = [(256, 8), (2048, 2), (4096, 4)]


def _nan_inputs(bank, N, P):
    C = 3
    W, per = bank.chunk(N), 4096 // N
    F = max(2 * per + 1, P + 3)
    assert per == 1 or C * F % per, "a ragged last tile"
    rng = np.random.default_rng([N, P, bank.real, 3])
    return rng, C, F, bank.rand(rng, (C, (F + P - 1) * W + 6)), bank.taps(rng, N, P)


def test_nan_sample_reaches_exactly_its_frames(sm, bank):
    for N, P in NAN_SHAPES:
        for power in MODES:
            _nan_sample(sm, bank, N, P, power)


def _nan_sample(sm, bank, N, P, power):
    rng, C, F, x, h = _nan_inputs(bank, N, P)
    W = bank.chunk(N)
    clean = bank.run(sm, x, h, N, power)
    for c in range(C):
        for j in (0, P - 1, P + 1, F + P - 2):
            for poison in (np.nan, np.inf):
                for half in ((0, 1) if bank.real else (0,)):
                    dirty_x = x.copy()
                    at = j * W + (2 * int(rng.integers(N)) + half if bank.real else int(rng.integers(N)))
                    dirty_x[c, at] = poison if bank.real else complex(poison, x[c, at].imag)
                    got = bank.run(sm, dirty_x, h, N, power, finite=False)
                    lo, hi = max(0, j - P + 1), min(j, F - 1)
                    what = f"{bank.name} N={N} P={P} power={power}: {poison} at sample {at} (chunk {j}) of stream {c}"
                    assert _non_finite(got[c, lo:hi + 1]).all(), what + f": frames {lo} ... {hi} are not non-finite in every element"
                    expect = _bits(clean).reshape(C, F, -1).copy()
                    seen = _bits(got).reshape(C, F, -1).copy()
                    expect[c, lo:hi + 1] = seen[c, lo:hi + 1] = 0
                    same = np.all(seen == expect, axis=-1)
                    assert same.all(), what + f": frames (stream, index) {np.argwhere(~same)[:8].tolist()} changed"


def test_nan_tap_reaches_every_frame(sm, bank):
    for N, P in NAN_SHAPES:
        for power in MODES:
            _nan_tap(sm, bank, N, P, power)


def _nan_tap(sm, bank, N, P, power):
    rng, C, F, x, h = _nan_inputs(bank, N, P)
    bank.run(sm, x, h, N, power)                       # the clean run is finite and writes every element (the guarded run)
    for t in (0, int(rng.integers(h.size)), h.size - 1):
        dirty_h = h.copy()
        dirty_h[t] = np.nan
        got = bank.run(sm, x, dirty_h, N, power, finite=False)
        bad = ~_non_finite(got)
        assert not bad.any(), f"{bank.name} N={N} P={P} power={power}: NaN tap {t} left elements (stream, frame, k) {np.argwhere(bad)[:8].tolist()} finite"

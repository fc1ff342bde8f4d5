"""The integrated power spectra (libsmfft_pfb_spec.so) per output spectrum and in isolation, on an MI355X: the ten kernels of
tests/pfb_spec_inventory.py, by bank and length.  Every run goes through the guarded run of tests/pfb_gpu_harness.py (Spectra.run: a
NaN-fenced signal into a prefilled, guarded output).  The probes are functions probe_*(sm, spec, N, real), spec the harness's Spectra,
listed in PROBES; they are run, at every length in both banks, by the one test of the library,
tests/test_pfb_spec_gpu.py::test_integrated_spectra (that module says why it is one test).  A plain module: no tests, no fixtures.

B1  Non-finite values reach exactly their spectra (probe_nan_sample_reaches_exactly_its_spectra, probe_nan_tap_reaches_every_spectrum).
    A NaN at one sample of block b of stream c (a block = one hop: N complex or 2N real samples) is inside frames b - P + 1 ... b,
    hence inside the integrations floor(f / T) of those frames that are computed (f < I T): every channel of exactly those spectra of
    that stream is NaN, and every other output word is what the clean run wrote, to the bit -- the first block, the last block of the
    first window, a block whose frames lie in two integrations, the last block a stream reads (the next stream's spectrum 0 stays
    clean; in the last stream the clamped slots of the ragged last tile load the poisoned group again and must store nothing: the guard
    of the run).  A NaN tap makes every channel of every spectrum NaN.  NaN is data here: nothing faults.
B2  Spectra are independent of where they are computed (probe_periodic_signal_gives_equal_bits): a Gaussian sequence of period T hops
    repeated along three streams makes every integration see the same samples, so every spectrum must equal the first one to the bit,
    across slots, tiles and streams, with a ragged last tile; the first one meets the model.
B3  Exact homogeneity (probe_doubling_the_signal_quadruples_the_output): the signal times 2 gives the output times 4 to the bit --
    scaling by a power of two commutes with every rounding of the weighted sum, the transform, the power and the sum."""
import numpy as np

from tests.pfb_gpu_harness import bits, chunk as _chunk, length, rand


def _name(real):
    return "real" if real else "complex"


def _taps(rng, N, P, real):
    return rng.standard_normal(P * _chunk(N, real)).astype(np.float32)


def probe_nan_sample_reaches_exactly_its_spectra(sm, spec, N, real):
    rng = np.random.default_rng(60 * N + real)
    per = 4096 // N
    P, T, C = 3, 2, 2
    n = per + 1                                  # a ragged second tile in the last stream, tiles straddling the streams
    chunk = _chunk(N, real)
    x, h = rand(rng, (C, length(N, P, n * T + 1, 0, real)), real), _taps(rng, N, P, real)
    clean = spec.run(sm, x, h, N, T, real)
    assert clean.shape == (C, n, N)
    last_block = n * T + P - 2                   # the last block a stream reads
    for c, b, pos in ((0, 0, 0), (0, P - 1, chunk - 1), (1, 3, chunk // 2 + 1), (0, last_block, 5), (1, last_block, chunk - 2)):
        bad = x.copy()
        bad[c, b * chunk + pos] = np.nan
        got = spec.run(sm, bad, h, N, T, real, finite=False)
        hit = sorted({f // T for f in range(max(0, b - P + 1), b + 1) if f < n * T})
        assert hit, (b, n, T)
        for i in range(n):
            for cc in range(C):
                if cc == c and i in hit:
                    assert np.all(np.isnan(got[cc, i])), f"{_name(real)} N={N}: NaN in block {b} of stream {c} did not reach all of spectrum {i}"
                else:
                    assert np.array_equal(bits(got[cc, i]), bits(clean[cc, i])), \
                        f"{_name(real)} N={N}: NaN in block {b} of stream {c} changed spectrum {i} of stream {cc}"


def probe_nan_tap_reaches_every_spectrum(sm, spec, N, real):
    rng = np.random.default_rng(61 * N + real)
    P, T, C = 3, 2, 2
    n = 4096 // N + 1
    x, h = rand(rng, (C, length(N, P, n * T, 0, real)), real), _taps(rng, N, P, real)
    for k in (0, h.size // 2 + 1, h.size - 1):
        bad = h.copy()
        bad[k] = np.nan
        got = spec.run(sm, x, bad, N, T, real, finite=False)
        assert got.shape == (C, n, N) and np.all(np.isnan(got)), f"{_name(real)} N={N}: NaN at tap {k}"


def probe_periodic_signal_gives_equal_bits(sm, spec, N, real):
    rng = np.random.default_rng(62 * N + real)
    per = 4096 // N
    P, T, C = 4, 3, 3
    n = 3 * per + 1 if per > 1 else 5
    chunk = _chunk(N, real)
    period = rand(rng, (T * chunk,), real)
    L = length(N, P, n * T, 0, real)
    one = np.tile(period, -(-L // period.size))[:L]
    x, h = np.stack([one] * C), _taps(rng, N, P, real)
    got = spec.run(sm, x, h, N, T, real)
    assert got.shape == (C, n, N)
    for c in range(C):
        for i in range(n):
            assert np.array_equal(bits(got[c, i]), bits(got[0, 0])), f"{_name(real)} N={N}: spectrum {i} of stream {c}"
    spec.check(got[:1, :1], x[:1, :(T + P - 1) * chunk], h, N, T, real, f"periodic {_name(real)} N={N}")


def probe_doubling_the_signal_quadruples_the_output(sm, spec, N, real):
    rng = np.random.default_rng(63 * N + real)
    P, T, C = 5, 4, 2
    n = 4096 // N + 1
    x, h = rand(rng, (C, length(N, P, n * T + 2, 0, real)), real), _taps(rng, N, P, real)
    base = spec.run(sm, x, h, N, T, real)
    twice = spec.run(sm, (2 * x).astype(x.dtype), h, N, T, real)
    assert np.array_equal(bits(twice), bits(4 * base)), f"{_name(real)} N={N}"


PROBES = (probe_nan_sample_reaches_exactly_its_spectra, probe_nan_tap_reaches_every_spectrum, probe_periodic_signal_gives_equal_bits,
          probe_doubling_the_signal_quadruples_the_output)

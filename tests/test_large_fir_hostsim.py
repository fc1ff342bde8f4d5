"""The overlap-save filter-bank kernels of include/smfft/smfft_large_fir.hpp run ON THE HOST, thread by thread, by the executor of
tests/hostsim (tests/hostsim/large_fir_host.cpp): the header's own segment loads, products, store windows and persistent loops -- the
recompute form at N = 8192 and 16384 and the held form at 8192, whichever the library ships -- against fp64, and whether their
barriers are sufficient.

1. every row against fp64 (`_reference` of tests/fir_gpu_harness.py, the tolerances and denominators of its `_check_rows`), on a host
   grid smaller than the unit count, with a NaN-prefilled output and guard bands around the three buffers;
2. the prepare kernel against fft(pad(g)) / N;
3. the same bits under every schedule;
4. a K-filter launch against K single-filter launches, and the held form against the recompute form: the same bits;
5. barrier knock-out against the table BARRIERS below.

The host library is built on demand into pytest's temporary directory."""
import ctypes
import os
import sys

import numpy as np
import pytest

from oracle.np_reference import MAX_ABS_TOL, REL_L2_TOL
from tests import fir_gpu_harness as fg
from tests import hostsim_harness as hh
from tests.hostsim_harness import GUARD, OUT_WORD, guarded as _guarded, payload as _payload, rand_complex as _rand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import large_fir_model as lfm  # noqa: E402

RECOMPUTE_8192, HELD_8192, RECOMPUTE_16384 = "large_fir<8192, 0>", "large_fir<8192, 1>", "large_fir<16384, 0>"
FORMS = (RECOMPUTE_8192, HELD_8192, RECOMPUTE_16384)
MODES = ("convolve", "correlate")

# ---- item 5: every barrier of one period of the filter loop, in program order ---------------------------------------------------------
# The recompute form's period is one unit: the six barriers of the forward transform and the six of the inverse one.  The held form's
# is one unit of two filters: forward, inverse, inverse.  `needed`: the run without it differs from the shipped run under some
# schedule.  All are: the six of a transform for the reasons of tests/test_large_hostsim.py (_C2C), and the sixth separates a
# transform's read of exchange C (thread u reads u + T*i) from the next transform's write of exchange A (thread u writes q*SA + u,
# other threads' slots) -- whether that next transform is the inverse one of the same unit, the next filter's, or the next unit's
# forward one.
_TRANSFORM = ["needed"] * 6
BARRIERS = {RECOMPUTE_8192: _TRANSFORM * 2, RECOMPUTE_16384: _TRANSFORM * 2, HELD_8192: _TRANSFORM * 3}


def _n(name):
    return int(name.split("<")[1].split(",")[0])


def _held(name):
    return name == HELD_8192


class FirHost:
    def __init__(self, path):
        self.lib = lib = ctypes.CDLL(path)
        vp, i, ll, ull, lng = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_long
        lib.hostsim_large_fir_run.argtypes = [ctypes.c_char_p, vp, vp, vp, ll, i, i, i, i, i, i, i, ull, i, i, i, lng, ctypes.POINTER(lng),
                                              ctypes.POINTER(ll)]
        lib.hostsim_large_fir_prepare.argtypes = [ctypes.c_char_p, vp, i, i, i, vp, i, i, ull, lng, ctypes.POINTER(lng)]
        lib.hostsim_large_fir_last_error.restype = ctypes.c_char_p

    def prepare(self, n, h, mode, grid=2):
        K, M = h.shape
        taps, t0 = _guarded(h)
        spec, s0 = _guarded(np.zeros((K, n), np.complex64), OUT_WORD)
        before = taps.copy()
        rc = self.lib.hostsim_large_fir_prepare(f"large_fir_prepare<{n}>".encode(), taps.ctypes.data + t0, M, K, int(mode == "correlate"),
                                                spec.ctypes.data + s0, grid, hh.ASC, 0, GUARD, None)
        assert rc == 0, self.lib.hostsim_large_fir_last_error().decode()
        assert np.array_equal(taps, before)
        return _payload(spec, s0, (K, n))

    def run(self, name, x, H, M, mode, group=1, grid=2, sched=hh.ASC, seed=0, desc=0, knock_out=-1, period=0):
        """-> ((C, K, L) output, barriers per workgroup, units); the three buffers sit between guard bands, the output NaN-prefilled"""
        C, L = x.shape
        K = H.shape[0]
        xs, x0 = _guarded(x)
        hs, h0 = _guarded(H)
        ys, y0 = _guarded(np.zeros((C, K, L), np.complex64), OUT_WORD)
        before_x, before_h, before_y = xs.copy(), hs.copy(), ys.copy()
        bars = (ctypes.c_long * grid)()
        units = ctypes.c_longlong(0)
        rc = self.lib.hostsim_large_fir_run(name.encode(), xs.ctypes.data + x0, hs.ctypes.data + h0, ys.ctypes.data + y0, L, C, K, M,
                                            int(mode == "correlate"), group, grid, sched, seed, desc, knock_out, period, GUARD, bars,
                                            ctypes.byref(units))
        assert rc == 0, f"{name}: executor error {rc}: {self.lib.hostsim_large_fir_last_error().decode()}"
        assert np.array_equal(xs, before_x) and np.array_equal(hs, before_h), "the signal, the spectra or their guards changed"
        lo, hi = y0 // 4, y0 // 4 + C * K * L * 2
        assert np.array_equal(ys[:lo], before_y[:lo]) and np.array_equal(ys[hi:], before_y[hi:]), "a write outside the output"
        return _payload(ys, y0, (C, K, L)), list(bars), units.value


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the build that contracts, as the device does"""
    out = str(tmp_path_factory.mktemp("hostsim_fir"))
    return FirHost(hh.build(["large_fir_host.cpp"], "libsmfft_large_fir_hostsim.so", out, hh.fma_flags(), csrc_includes=True))


def _group(name, K):
    """the filters per unit a test gives the held form: two, so that K = 3 leaves an uneven last group"""
    return min(2, K) if _held(name) else 1


def _expected_barriers(name, units, grid, K, group):
    """6 per forward transform and 6 per filter of the unit; unit = segment * groups + g"""
    groups = -(-K // group)
    bars = [0] * grid
    for unit in range(units):
        g = unit % groups
        filters = min(K, (g + 1) * group) - g * group
        bars[unit % grid] += 6 + 6 * filters
    return bars


# ---- 1. every row against fp64 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", FORMS)
def test_host_filter_bank_matches_fp64(host, name, mode):
    n = _n(name)
    rng = np.random.default_rng([n, _held(name), mode == "correlate"])
    worst = (0.0, 0.0)
    for M in (1, 17, n // 4 + 1, n - 1):
        V = n - M + 1
        # L < M (M / 2; at M = N - 1, where that would be thousands of two-output segments, V + 1: two segments); exactly V; 2 V - 3;
        # and for M = N - 1 forty segments
        lengths = [min(max(1, M // 2), V + 1), V, 2 * V - 3] + ([2 * 40] if M == n - 1 else [])
        for L in lengths:
            if L < 1:
                continue
            for C, K in ((1, 1), (2, 3)):
                x, h = _rand(rng, (C, L)), _rand(rng, (K, M))
                H = host.prepare(n, h, mode)
                group = _group(name, K)
                units = lfm.Window(L, n, M, mode == "correlate").segments() * C * -(-K // group)
                grid = max(1, min(3, units - 1))              # smaller than the unit count: the persistent loop wraps
                got, bars, ran = host.run(name, x, H, M, mode, group=group, grid=grid)
                assert ran == units and bars == _expected_barriers(name, units, grid, K, group), (name, M, L, C, K, bars)
                assert np.isfinite(got.view(np.float32)).all(), "outputs left unwritten"
                want = fg._reference(x, h, mode == "correlate")
                fg._check_rows(got, want, f"{name} {mode} M={M} L={L} C={C} K={K}", x, h)
                d = got - want
                worst = (max(worst[0], np.linalg.norm(d) / np.linalg.norm(want)), max(worst[1], np.abs(d).max() / np.abs(want).max()))
    print(f"{name} {mode}: worst whole-case relL2 {worst[0]:.2e}, max {worst[1]:.2e}")


def test_forty_segments_case_has_forty_segments():
    for n in (8192, 16384):
        assert lfm.Window(80, n, n - 1, False).segments() == 40


# ---- 2. the prepare kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (8192, 16384))
def test_host_prepare_matches_fp64(host, n):
    rng = np.random.default_rng(n)
    for mode in MODES:
        for M in (1, 17, n // 4 + 1, n - 1):
            h = _rand(rng, (3, M))                  # three filters on a grid of two: the loop wraps
            got = host.prepare(n, h, mode)
            want = lfm.spectra(h, n, mode == "correlate")
            for k in range(3):
                d = got[k] - want[k]
                l2, mx = np.linalg.norm(d) / np.linalg.norm(want[k]), np.abs(d).max() / np.abs(want[k]).max()
                assert l2 <= REL_L2_TOL and mx <= MAX_ABS_TOL, (n, mode, M, k, l2, mx)


# ---- the case of items 3-5: two segments, two filters ---------------------------------------------------------------------------------------
def _small_case(name, mode="convolve", K=2):
    n = _n(name)
    M = n // 4 + 1
    L = 2 * (n - M + 1) - 3
    rng = np.random.default_rng([n, 5, K])
    x, h = _rand(rng, (1, L)), _rand(rng, (K, M))
    return n, M, x, h


# ---- 3. schedule invariance ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FORMS)
def test_host_schedule_invariance(host, name):
    n, M, x, h = _small_case(name)
    H = host.prepare(n, h, "convolve")
    group = _group(name, 2)
    base, bars, units = host.run(name, x, H, M, "convolve", group=group, grid=1)
    assert bars == _expected_barriers(name, units, 1, 2, group)
    for sched, seed, desc in hh.SCHEDULES:
        got, b, _ = host.run(name, x, H, M, "convolve", group=group, grid=2 if not _held(name) else 1, sched=sched, seed=seed, desc=desc)
        assert hh.same(got, base), f"{name}: schedule {sched} seed {seed} workgroups descending={desc} changes the bits"
        assert sum(b) == sum(bars)


# ---- 4. filter groups and forms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", FORMS)
def test_host_k_filters_equal_k_single_launches(host, name, mode):
    n, M, x, h = _small_case(name, mode, K=3)
    H = host.prepare(n, h, mode)
    got, _, _ = host.run(name, x, H, M, mode, group=_group(name, 3), grid=2)
    for k in range(3):
        one, _, _ = host.run(name, x, H[k:k + 1], M, mode, grid=1)
        assert hh.same(one[0, 0], got[0, k]), (name, mode, k)


@pytest.mark.parametrize("mode", MODES)
def test_host_held_equals_recompute(host, mode):
    """the same arithmetic per output element in both forms: the same bits, for groups of 1, 2 and 3 filters"""
    n, M, x, h = _small_case(HELD_8192, mode, K=3)
    H = host.prepare(n, h, mode)
    want, _, _ = host.run(RECOMPUTE_8192, x, H, M, mode, grid=2)
    for group in (1, 2, 3):
        got, _, _ = host.run(HELD_8192, x, H, M, mode, group=group, grid=2)
        assert hh.same(got, want), (mode, group)


# ---- 5. barrier knock-out ------------------------------------------------------------------------------------------------------------------------
def test_barrier_table_is_complete():
    assert set(BARRIERS) == set(FORMS)
    for name, table in BARRIERS.items():
        assert len(table) == (18 if _held(name) else 12), name
        assert all(e == "needed" or (e.startswith("redundant: ") and len(e) > 80) for e in table), name


@pytest.mark.parametrize("name", FORMS)
def test_host_barrier_knock_out(host, name):
    """One workgroup runs every unit of the small case (two segments x two filters: four units of the recompute form, two of the held
    form with both filters in one group), so every barrier of the period is followed by another transform on the same image.  For every
    `needed` barrier the run without it differs from the shipped run under some schedule; a `redundant` one is bit-identical under all."""
    table = BARRIERS[name]
    period = len(table)
    n, M, x, h = _small_case(name)
    H = host.prepare(n, h, "convolve")
    group = _group(name, 2)

    def run_base():
        base, bars, units = host.run(name, x, H, M, "convolve", group=group, grid=1)
        assert bars == [period * units]
        return base, bars
    hh.knock_out(table, run_base, lambda k, sched, seed, desc: host.run(name, x, H, M, "convolve", group=group, grid=1, sched=sched, seed=seed, desc=desc,
                                                                        knock_out=k, period=period)[:2], name)

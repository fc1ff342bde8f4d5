"""The polyphase filter bank kernels of include/smfft/smfft_large_pfb.hpp run ON THE HOST, thread by thread, by the executor of
tests/hostsim (tests/hostsim/large_pfb_host.cpp): the header's own tap loop, schedule, transform and stores -- both modes at N = 8192
and 16384 -- against fp64, and whether their barriers are sufficient.

1. every row against fp64 (tools/large_pfb_model.py, the row bounds of tests/pfb_gpu_harness.py: complex ||d||_2 / (sqrt(N) ||s||_2) <= 1e-6
   and max <= 5e-6, power L1 <= 2e-6 and max <= 1e-5), with a NaN-prefilled output and guard bands around the three buffers.  Shapes:
   P in {1, 3}, two streams, three full rounds of the grid and a ragged one -- 26 pairs on a host grid of 8 under both schedules
   (two streams make the pair count even: 3 G + 2), 10 pairs on a grid of 3 under the stride schedule (3 G + 1; the blocked form needs
   a grid of at least 8 and falls back to the stride form below it);
2. both schedules and grids of 1, 3, 8 and 16 give the same bits (at G = 8, the grid of item 1, the blocked schedule assigns the pairs
   as the stride schedule does; it permutes them at G = 16);
3. the same bits under every order of the threads and of the workgroups;
4. a two-stream launch against two one-stream launches;
5. barrier knock-out with period six: each of the engine's six barriers is needed.

The host library is built on demand into pytest's temporary directory.  The file's wall time is printed at the end of the module."""
import ctypes
import os
import sys
import time

import numpy as np
import pytest

from tests import hostsim_harness as hh
from tests import pfb_gpu_harness as gh
from tests.hostsim_harness import GUARD, OUT_WORD, guarded as _guarded, rand_complex as _rand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import large_pfb_model as lpm  # noqa: E402

SIZES = (8192, 16384)
STRIDE, BLOCKED = 1, 2
# (host grid, kernel schedule, frames per stream of the two streams)
GRIDS = ((8, STRIDE, 13), (8, BLOCKED, 13), (3, STRIDE, 5))

# ---- item 5: the six barriers of one pair, in program order (the table of tests/test_large_hostsim.py, _C2C).  The tap loop between two
# transforms touches no LDS, so the sixth still separates read_c (thread u reads u + T*i) from the next pair's write of exchange A
# (thread u writes q*SA + u: other threads' slots).
BARRIERS = ["needed"] * 6
BANK = gh.Bank("large_pfb")      # the bank's row checks; the library itself is not loaded here


class PfbHost:
    def __init__(self, path):
        self.lib = lib = ctypes.CDLL(path)
        vp, i, ll, ull, lng = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_long
        lib.hostsim_large_pfb_run.argtypes = [i, i, vp, vp, vp, ll, i, i, i, i, i, ull, i, i, i, lng, ctypes.POINTER(lng), ctypes.POINTER(i)]
        lib.hostsim_large_pfb_last_error.restype = ctypes.c_char_p

    def run(self, n, x, h, power, form=STRIDE, grid=3, sched=hh.ASC, seed=0, desc=0, knock_out=-1, period=0):
        """-> ((C, F, N) output, barriers per workgroup, (grid, form) as launched); the three buffers sit between guard bands, the
        output NaN-prefilled"""
        C, L = x.shape
        P = h.size // n
        F = lpm.frames(L, n, P)
        dtype = np.float32 if power else np.complex64
        xs, x0 = _guarded(x)
        hs, h0 = _guarded(h)
        ys, y0 = _guarded(np.zeros((C, F, n), dtype), OUT_WORD)
        before_x, before_h, before_y = xs.copy(), hs.copy(), ys.copy()
        bars = (ctypes.c_long * grid)()
        launched = (ctypes.c_int * 2)()
        rc = self.lib.hostsim_large_pfb_run(n, int(power), xs.ctypes.data + x0, hs.ctypes.data + h0, ys.ctypes.data + y0, L, C, P, form, grid, sched, seed,
                                            desc, knock_out, period, GUARD, bars, launched)
        assert rc == 0, f"pfb_large<{n}, {int(power)}>: executor error {rc}: {self.lib.hostsim_large_pfb_last_error().decode()}"
        assert np.array_equal(xs, before_x) and np.array_equal(hs, before_h), "the signal, the taps or their guards changed"
        words = C * F * n * (1 if power else 2)
        lo, hi = y0 // 4, y0 // 4 + words
        assert np.array_equal(ys[:lo], before_y[:lo]) and np.array_equal(ys[hi:], before_y[hi:]), "a write outside the output"
        return hh.payload(ys, y0, (C, F, n), dtype), list(bars)[:launched[0]], tuple(launched)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the build that contracts, as the device does"""
    started = time.time()
    out = str(tmp_path_factory.mktemp("hostsim_large_pfb"))
    lib = hh.build(["large_pfb_host.cpp"], "libsmfft_large_pfb_hostsim.so", out, hh.fma_flags(), csrc_includes=True)
    yield PfbHost(lib)
    print(f"\ntests/test_large_pfb_hostsim.py: {time.time() - started:.1f} s of wall time, the build of the host library included")


def _expected_barriers(pairs, grid, form):
    sched = lpm.Schedule(pairs, grid, form)
    return [6 * len(sched.pairs_of(b)) for b in range(grid)]


# ---- 1. and 2. every row against fp64; the same bits under both schedules and both grids ------------------------------------------------
@pytest.mark.parametrize("power", (False, True))
@pytest.mark.parametrize("P", (1, 3))
@pytest.mark.parametrize("n", SIZES)
def test_host_filter_bank_matches_fp64(host, n, P, power):
    runs = {}
    rng = np.random.default_rng([n, P])          # the same inputs in both modes
    taps = rng.standard_normal(P * n).astype(np.float32)
    for F in sorted({f for _, _, f in GRIDS}):
        L = (F + P - 1) * n + 37                   # a ragged tail that no frame reads
        x = _rand(rng, (2, L))
        ref = lpm.pfb(x, taps, n)
        s = lpm.scale(x, taps, n)
        assert ref.shape == (2, F, n)
        for grid, form, frames in GRIDS:
            if frames != F:
                continue
            pairs = 2 * F
            assert pairs == 3 * grid + (2 if grid == 8 else 1)
            got, bars, launched = host.run(n, x, taps, power, form=form, grid=grid)
            assert launched == (grid, form) and bars == _expected_barriers(pairs, grid, form), (n, P, grid, form, bars)
            assert np.isfinite(got.view(np.float32)).all(), "outputs left unwritten"
            what = f"host N={n} P={P} grid={grid} schedule={form}"
            BANK.check(got, ref, s, power, what + (" power" if power else ""))
            runs[(grid, form)] = got
    # the blocked form at G = 8 assigns the pairs as the stride form does, so this holds the form's own code path to the same bits, no more
    # (a real permutation: test_host_grids_and_schedules_give_the_same_bits)
    assert hh.same(runs[(8, STRIDE)], runs[(8, BLOCKED)]), (n, P, power, "stride and blocked schedules differ")


@pytest.mark.parametrize("n", SIZES)
def test_host_grids_and_schedules_give_the_same_bits(host, n):
    """one shape (P = 3, two streams of 9 frames: 18 pairs) on a grid of 1, of 3 (stride), and of 8 and 16 under both schedules.  At
    G = 8 the blocked form is the identity (slot(b) = b for b < 8); at G = 16 it is a permutation, slot(b) = 2 (b mod 8) + b / 8, so this
    is the host run in which a pair is computed by another workgroup, in another round, than under the stride form."""
    P, F = 3, 9
    rng = np.random.default_rng([n, 7])
    x, taps = _rand(rng, (2, (F + P - 1) * n + 3)), rng.standard_normal(P * n).astype(np.float32)
    for power in (False, True):
        base, bars, _ = host.run(n, x, taps, power, grid=1)
        assert bars == [108]
        for grid, form in ((3, STRIDE), (8, STRIDE), (8, BLOCKED), (16, STRIDE), (16, BLOCKED)):
            got, bars, launched = host.run(n, x, taps, power, form=form, grid=grid)
            assert launched == (grid, form) and bars == _expected_barriers(18, grid, form)
            assert hh.same(got, base), (n, power, grid, form)
        # a grid below 8 falls back to the stride form
        got, _, launched = host.run(n, x, taps, power, form=BLOCKED, grid=7)
        assert launched == (7, STRIDE) and hh.same(got, base)


# ---- the case of items 3 and 5: three pairs of two taps -----------------------------------------------------------------------------------
def _small_case(n):
    P, F = 2, 3
    rng = np.random.default_rng([n, 5])
    return _rand(rng, (1, (F + P - 1) * n)), rng.standard_normal(P * n).astype(np.float32)


# ---- 3. schedule invariance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_host_schedule_invariance(host, n):
    x, taps = _small_case(n)
    base, bars, _ = host.run(n, x, taps, False, grid=1)
    assert bars == [18]
    for sched, seed, desc in hh.SCHEDULES:
        got, b, _ = host.run(n, x, taps, False, grid=2, sched=sched, seed=seed, desc=desc)
        assert hh.same(got, base), f"N={n}: schedule {sched} seed {seed} workgroups descending={desc} changes the bits"
        assert b == [12, 6]


# ---- 4. streams ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_host_two_streams_equal_two_launches(host, n):
    P, F = 2, 3
    rng = np.random.default_rng([n, 9])
    x, taps = _rand(rng, (2, (F + P - 1) * n + 11)), rng.standard_normal(P * n).astype(np.float32)
    for power in (False, True):
        together, _, _ = host.run(n, x, taps, power, grid=4)      # pairs straddle the streams in every round
        for c in range(2):
            alone, _, _ = host.run(n, x[c:c + 1], taps, power, grid=2)
            assert hh.same(alone[0], together[c]), (n, power, c)


# ---- 5. barrier knock-out ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_host_barrier_knock_out(host, n):
    """One workgroup runs the three pairs of the small case, so every barrier of the period is followed by another transform on the same
    image.  For every barrier the run without it differs from the shipped run under some schedule."""
    assert len(BARRIERS) == 6 and all(e == "needed" for e in BARRIERS)
    x, taps = _small_case(n)

    def run_base():
        base, bars, _ = host.run(n, x, taps, False, grid=1)
        assert bars == [18]
        return base, bars
    hh.knock_out(BARRIERS, run_base, lambda k, sched, seed, desc: host.run(n, x, taps, False, grid=1, sched=sched, seed=seed, desc=desc, knock_out=k, period=6)[:2],
                 f"pfb_large<{n}, 0>")

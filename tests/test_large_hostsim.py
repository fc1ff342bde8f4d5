"""The eight single-pass large kernels (include/smfft/smfft_large.hpp, smfft_large_real.hpp) run ON THE HOST, thread by thread, by the
executor of tests/hostsim: the headers' own butterflies, LDS addressing and persistent loops against fp64, and -- what no GPU run can
show -- whether their barriers are sufficient.  One kernel thread runs at a time, in an order a schedule chooses for every barrier
interval, so a run is a deterministic function of (kernel, inputs, schedule, seed): two threads that touch one LDS slot in one interval
give different bits under the schedules `ascending` and `descending`, which order every pair both ways.

1. the arithmetic against fp64 (per-FFT tolerances of oracle/np_reference.py, per-element probe ceiling of tests/test_probes_gpu.py), on a
   host build without contraction and on one with contraction and FMA;
2. schedule invariance of the shipped barriers, out of place and in place;
3. the persistent loop: rows against single launches, a NaN row, the LDS prefill;
4. guarded buffers at interior pointers, nFFTs of 0, 1 and fewer than the grid;
5. barrier knock-out against the table BARRIERS below;
6. the executor's own checks on toy kernels with known faults.

The host library is built on demand into pytest's temporary directory."""
import ctypes
import math

import numpy as np
import pytest

from oracle import np_reference as ref
from tests import hostsim_harness as hh
from tests.hostsim_harness import ASC, DESC, GUARD, GUARD_WORD, RANDOM, SCHEDULES
from tests.hostsim_harness import bits as _bits, same as _same

G = 3                      # host grid
NFFTS = 3 * G + 1          # three full rounds and a ragged one: workgroup 0 carries its image three times

# ---- item 5: every barrier of every kernel's loop, in program order ------------------------------------------------------------------
# `needed`: the run without it differs from the shipped run under some schedule.  `redundant: reason`: bit-identical under all
# schedules, and the reason says which thread touches which slots in the two intervals the barrier separates (checked by hand against
# the header).  Filled from what the host run shows.
_C2C = ["needed",     # exchange A written (q*SA + u) | read by other threads (lds_a(u) + 64i)
        "needed",     # exchange A read | exchange B written over it
        "needed",     # exchange B written | read by other threads
        "needed",     # exchange B read | exchange C written over it
        "needed",     # exchange C written | read by other threads
        "needed"]     # exchange C read (u + T*i) | the next FFT's exchange A written at q*SA + u: other threads' slots
_OWN_SLOTS = ("redundant: before it read_c has thread u read lds[u + T*i], i < 16; after it LargeRealSplit::write has thread u write "
              "lds[u + T*q], q < 16 -- the same sixteen slots, its own -- and thread 0 lds[L], which read_c never reads (u + 15T <= L - 1); "
              "pass4 between them touches no LDS")
BARRIERS = {
    "large_c2c<8192, 0>": _C2C, "large_c2c<8192, 1>": _C2C, "large_c2c<16384, 0>": _C2C, "large_c2c<16384, 1>": _C2C,
    # R2C: the six of the C2C loop, then exchange S written | partner read | next FFT's exchange A
    "large_r2c<16384>": _C2C[:5] + [_OWN_SLOTS, "needed", "needed"],
    "large_r2c<32768>": _C2C[:5] + [_OWN_SLOTS, "needed", "needed"],
    # C2R: exchange S written | partner read | exchange A ... exchange C read | the NEXT FFT's exchange S written
    "large_c2r<16384>": ["needed", "needed"] + _C2C[:5] + [_OWN_SLOTS],
    "large_c2r<32768>": ["needed", "needed"] + _C2C[:5] + [_OWN_SLOTS],
}
KERNELS = sorted(BARRIERS)


def _kind(name):
    """(r2c | c2r | c2c, transform length N, inverse)"""
    head, args = name.rstrip(">").split("<")
    a = [int(v) for v in args.split(",")]
    return head[len("large_"):], a[0], bool(a[1]) if len(a) > 1 else head.endswith("c2r")


# ---- the host library ---------------------------------------------------------------------------------------------------------------
class HostLib:
    def __init__(self, path):
        self.lib = lib = ctypes.CDLL(path)
        tail = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.POINTER(ctypes.c_long)]
        lib.hostsim_large_run.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p] + tail
        lib.hostsim_toy_run.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p] + tail
        lib.hostsim_last_error.restype = lib.hostsim_toy_last_error.restype = ctypes.c_char_p
        lib.hostsim_lds_prefill.restype = ctypes.c_uint

    def run_raw(self, name, src, dst, nffts, grid=G, sched=ASC, seed=0, desc=0, knock_out=-1, period=0, guard=0):
        """-> (error code, message, barriers per workgroup)"""
        bars = (ctypes.c_long * max(grid, 1))()
        rc = self.lib.hostsim_large_run(name.encode(), src, dst, nffts, grid, sched, seed, desc, knock_out, period, guard, bars)
        return rc, self.lib.hostsim_last_error().decode(), list(bars)[:grid]

    def run(self, name, x, in_place=False, **kw):
        """-> (output array, barriers per workgroup); any executor error fails the test"""
        kind, n, _ = _kind(name)
        nffts = x.shape[0]
        if in_place:
            buf = x.copy()
            rc, msg, bars = self.run_raw(name, buf.ctypes.data, buf.ctypes.data, nffts, **kw)
            out = buf.reshape(-1).view(_out_dtype(kind)).reshape(_out_shape(kind, n, nffts))
        else:
            out = np.zeros(_out_shape(kind, n, nffts), _out_dtype(kind))
            rc, msg, bars = self.run_raw(name, x.ctypes.data, out.ctypes.data, nffts, **kw)
        assert rc == 0, f"{name}: executor error {rc}: {msg}"
        return out, bars

    def toy(self, fault, x, out, rounds, grid=1, sched=ASC, seed=0, desc=0, knock_out=-1, period=0, guard=0):
        bars = (ctypes.c_long * max(grid, 1))()
        rc = self.lib.hostsim_toy_run(fault, x, out, rounds, grid, sched, seed, desc, knock_out, period, guard, bars)
        return rc, self.lib.hostsim_toy_last_error().decode(), list(bars)[:grid]


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    base = tmp_path_factory.mktemp("hostsim")
    flags = {"strict": ["-ffp-contract=off"], "fma": hh.fma_flags()}
    return {k: HostLib(hh.build(["large_host.cpp", "toy_kernels.cpp"], "libsmfft_large_hostsim.so", str(base / k), f)) for k, f in flags.items()}


@pytest.fixture(scope="module")
def host(builds):
    """the build that contracts, as the device does: items 2-6 are about order and addresses, not rounding"""
    return builds["fma"]


# ---- data ---------------------------------------------------------------------------------------------------------------------------
def _out_dtype(kind):
    return np.float32 if kind == "c2r" else np.complex64


def _out_shape(kind, n, nffts):
    return (nffts, n) if kind != "r2c" else (nffts, n // 2)


def _gaussian(name, nffts, seed=0):
    kind, n, _ = _kind(name)
    rng = np.random.default_rng([n, seed, len(kind)])
    if kind == "r2c":
        return rng.standard_normal((nffts, n)).astype(np.float32)
    m = n // 2 if kind == "c2r" else n
    return (rng.standard_normal((nffts, m)) + 1j * rng.standard_normal((nffts, m))).astype(np.complex64)


def _fp64(name, x):
    kind, n, inverse = _kind(name)
    if kind == "r2c":
        return ref.r2c_packed(x)
    if kind == "c2r":
        return ref.c2r_packed(x)
    x = x.astype(np.complex128)
    return np.fft.ifft(x, axis=1) * n if inverse else np.fft.fft(x, axis=1)


def _rows_of(wg, nffts, grid=G):
    return len(range(wg, nffts, grid))


def _assert_barrier_counts(name, bars, nffts, grid=G):
    """the case-count condition: the loop executes exactly the table's number of barriers per FFT"""
    period = len(BARRIERS[name])
    assert bars == [period * _rows_of(wg, nffts, grid) for wg in range(grid)], (name, bars)


# ---- 1. the header's arithmetic against fp64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", ["strict", "fma"])
@pytest.mark.parametrize("name", KERNELS)
def test_host_matches_fp64(builds, name, build):
    x = _gaussian(name, NFFTS)
    got, bars = builds[build].run(name, x)
    _assert_barrier_counts(name, bars, NFFTS)
    want = _fp64(name, x)
    for f in range(NFFTS):
        l2, mx = ref.fft_errors(got[f], want[f])
        print(f"{name} {build} FFT {f}: relL2={l2:.3e} maxabs={mx:.3e}")
        assert l2 <= ref.REL_L2_TOL and mx <= ref.MAX_ABS_TOL, f"{name} {build} FFT {f}: relL2={l2:.3e} maxabs={mx:.3e}"


def _probe_rows(name):
    """the probes of tests/test_large_gpu.py / test_large_real_gpu.py: positions 0, 1, N/2 - 1, N/2, N - 1 and 40 seeded ones"""
    kind, n, _ = _kind(name)
    if kind == "c2r":
        L = n // 2
        rng = np.random.default_rng(13)
        bins = np.unique(np.concatenate([[1, L // 2 - 1, L // 2, L - 1], rng.integers(1, L, 40)]))
        rows = [(0, 1.0 + 0j), (0, 1j)]          # DC alone, Nyquist alone (element 0's imaginary part)
        for k in bins:
            rows += [(k, 1.0 + 0j), (k, np.exp(2j * np.pi * rng.random()))]
        x = np.zeros((len(rows), L), dtype=np.complex64)
        for r, (k, v) in enumerate(rows):
            x[r, k] = v
        return x
    rng = np.random.default_rng(11)
    pos = np.unique(np.concatenate([[0, 1, n // 2 - 1, n // 2, n - 1], rng.integers(0, n, 40)]))
    x = np.zeros((len(pos), n), dtype=np.float32 if kind == "r2c" else np.complex64)
    x[np.arange(len(pos)), pos] = 1
    return x


@pytest.mark.parametrize("build", ["strict", "fma"])
@pytest.mark.parametrize("name", KERNELS)
def test_host_dft_matrix_probe(builds, name, build):
    """Unit impulses (C2C, R2C) / single bins (C2R): every output element is one entry of the DFT matrix; its error, per element and as
    rms, stays under the twiddle-chain ceiling 3 (log2 N + 2) 2^-24 that tests/test_probes_gpu.py derives for any correctly rounded
    fp32 evaluation order."""
    _, n, _ = _kind(name)
    x = _probe_rows(name)
    got, _ = builds[build].run(name, x)
    err = np.abs(got.astype(np.complex128 if np.iscomplexobj(got) else np.float64) - _fp64(name, x))
    ceiling = 3 * (math.log2(n) + 2) * 2.0 ** -24
    rms = np.sqrt(np.mean(err ** 2))
    print(f"{name} {build}: per-element {err.max():.3e}, rms {rms:.3e}, ceiling {ceiling:.3e}")
    assert err.max() <= ceiling, f"{name} {build}: per-element {err.max():.3e} > {ceiling:.3e} (row {np.unravel_index(err.argmax(), err.shape)})"
    assert rms <= ceiling


# ---- 2. schedule invariance: no race with the barriers as shipped ------------------------------------------------------------------
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("name", KERNELS)
def test_host_schedule_invariance(host, name, in_place):
    x = _gaussian(name, NFFTS)
    base, _ = host.run(name, x)
    assert np.isfinite(base.view(np.float32)).all()
    counts = []
    for sched, seed, desc in SCHEDULES:
        got, bars = host.run(name, x, in_place=in_place, sched=sched, seed=seed, desc=desc)
        assert _same(got, base), f"{name}: schedule {sched} seed {seed} workgroups descending={desc} in_place={in_place} changes the bits"
        counts.append(bars)
    for bars in counts:
        _assert_barrier_counts(name, bars, NFFTS)


# ---- 3. the persistent loop ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KERNELS)
def test_host_persistent_loop(host, name):
    x = _gaussian(name, NFFTS, seed=3)
    base, _ = host.run(name, x)
    prefill = host.lib.hostsim_lds_prefill()
    assert np.isfinite(base.view(np.float32)).all() and not (_bits(base) == prefill).any(), "an LDS slot was read before it was written"
    for f in range(NFFTS):
        alone, bars = host.run(name, x[f:f + 1], grid=1)
        assert bars == [len(BARRIERS[name])]
        assert _same(alone[0], base[f]), f"{name}: FFT {f} of the batch differs from a launch of its own"
    # a NaN row: workgroup 0 transforms rows 0, G, 2G, 3G -- row G is poisoned and a clean row follows on the same image
    xn = x.copy()
    xn[G] = np.nan
    got, _ = host.run(name, xn)
    assert np.isnan(got[G].view(np.float32)).all(), "the NaN row does not reach all of its output row"
    clean = [f for f in range(NFFTS) if f != G]
    assert _same(got[clean], base[clean]), "the NaN row reaches another FFT's output"


# ---- 4. buffers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KERNELS)
def test_host_guarded_buffers(host, name):
    kind, n, _ = _kind(name)
    for nffts in (NFFTS, 0, 1, G - 1):
        x = _gaussian(name, max(nffts, 1), seed=9)[:nffts]
        nbytes = x.nbytes
        src, off = hh.guarded(x)
        dst, _ = hh.guarded(nbytes)
        before_src, before_dst = src.copy(), dst.copy()
        rc, msg, bars = host.run_raw(name, src.ctypes.data + off, dst.ctypes.data + off, nffts, guard=GUARD)
        assert rc == 0, f"{name} nFFTs={nffts}: {msg}"
        _assert_barrier_counts(name, bars, nffts)       # nFFTs < G: whole workgroups return before their first barrier
        assert np.array_equal(src, before_src), "the input buffer or its guards changed"
        lo, hi = off // 4, (off + nbytes) // 4
        assert np.array_equal(dst[:lo], before_dst[:lo]), "a write before the output"
        assert np.array_equal(dst[hi:], before_dst[hi:]), "a write past the output"
        if nffts:
            got = dst[lo:hi].view(_out_dtype(kind)).reshape(_out_shape(kind, n, nffts))
            assert np.isfinite(got.view(np.float32)).all(), "a guard value (or an unwritten output) reaches the output"
            assert _same(got, host.run(name, x)[0])


# ---- 5. barrier knock-out ---------------------------------------------------------------------------------------------------------------
def test_barrier_table_is_complete():
    for name, table in BARRIERS.items():
        assert len(table) == (6 if "c2c" in name else 8), name
        for entry in table:
            assert entry == "needed" or (entry.startswith("redundant: ") and len(entry) > 80), (name, entry)


@pytest.mark.parametrize("name", KERNELS)
def test_host_barrier_knock_out(host, name):
    """For every `needed` barrier the run without it differs from the shipped run under some schedule of item 2 -- so item 2 can see a
    missing barrier at that place; for every `redundant` one it is bit-identical under all of them."""
    table = BARRIERS[name]
    x = _gaussian(name, NFFTS)

    def run_base():
        base, bars = host.run(name, x)
        _assert_barrier_counts(name, bars, NFFTS)
        return base, bars
    hh.knock_out(table, run_base, lambda k, sched, seed, desc: host.run(name, x, sched=sched, seed=seed, desc=desc, knock_out=k, period=len(table)), name)


# ---- 6. the executor's own checks ----------------------------------------------------------------------------------------------------------
TOY_T, TOY_ROUNDS, TOY_GRID = 256, 3, 2
OK, DIVERGENT, LDS_OOB, GLOBAL_OOB = 0, 1, 2, 3


def _toy_buffers():
    n = TOY_T * TOY_ROUNDS * TOY_GRID
    src = np.full(n + GUARD // 2, GUARD_WORD, dtype=np.uint32)
    dst = src.copy()
    lo = GUARD // 8
    x = np.random.default_rng(6).standard_normal(n).astype(np.float32)
    src[lo:lo + n] = x.view(np.uint32)
    return x, src, dst, lo, n


def _toy(host, fault, **kw):
    x, src, dst, lo, n = _toy_buffers()
    rc, msg, bars = host.toy(fault, src.ctypes.data + 4 * lo, dst.ctypes.data + 4 * lo, TOY_ROUNDS, grid=TOY_GRID, guard=GUARD // 2, **kw)
    return rc, msg, bars, x, dst[lo:lo + n].view(np.float32).copy(), dst, lo, n


def test_executor_passes_a_correct_kernel(host):
    want = None
    for sched, seed, desc in SCHEDULES:
        rc, msg, bars, x, got, dst, lo, n = _toy(host, 0, sched=sched, seed=seed, desc=desc)
        assert rc == OK, msg
        assert bars == [2 * TOY_ROUNDS] * TOY_GRID
        want = x.reshape(-1, TOY_T)[:, ::-1].reshape(-1)
        assert np.array_equal(got, want)
        assert (dst[:lo] == GUARD_WORD).all() and (dst[lo + n:] == GUARD_WORD).all()
    # its two barriers are both needed: knocked out, some schedule shows it
    for k in (0, 1):
        rc, msg, bars, x, got, *_ = _toy(host, 0, sched=DESC, knock_out=k, period=2)
        assert rc == OK and bars == [2 * TOY_ROUNDS] * TOY_GRID
        assert not np.array_equal(got, want), f"knocking out barrier {k} of the toy kernel is not seen"


def test_executor_sees_a_missing_barrier(host):
    results = [_toy(host, 1, sched=sched, seed=seed, desc=desc) for sched, seed, desc in SCHEDULES]
    assert all(r[0] == OK for r in results)
    assert not all(np.array_equal(_bits(r[4]), _bits(results[0][4])) for r in results), "a racy kernel gives the same bits under every schedule"
    assert not np.array_equal(_bits(results[0][4]), _bits(results[1][4])), "ascending and descending agree on a pairwise race"


def test_executor_reports_divergent_barriers_and_early_exits(host):
    for fault in (2, 6):
        for sched in (ASC, DESC, RANDOM):
            rc, msg, *_ = _toy(host, fault, sched=sched, seed=1)
            assert rc == DIVERGENT and "barrier" in msg, (fault, rc, msg)


def test_executor_shows_a_read_of_unwritten_lds(host):
    rc, msg, bars, x, got, *_ = _toy(host, 3)
    assert rc == OK
    assert (_bits(got) == host.lib.hostsim_lds_prefill()).all() and np.isnan(got).all()


def test_executor_reports_writes_out_of_bounds(host):
    rc, msg, *_ = _toy(host, 4)
    assert rc == LDS_OOB and "LDS" in msg, (rc, msg)
    rc, msg, *_ = _toy(host, 5)
    assert rc == GLOBAL_OOB and "guard" in msg, (rc, msg)


def test_executor_rejects_bad_launches(host):
    x = _gaussian(KERNELS[0], 1)
    out = np.zeros_like(x)
    assert host.run_raw("large_c2c<4096, 0>", x.ctypes.data, out.ctypes.data, 1)[0] == -1
    assert host.run_raw(KERNELS[0], x.ctypes.data, out.ctypes.data, 1, sched=7)[0] == 4
    assert host.run_raw(KERNELS[0], x.ctypes.data, out.ctypes.data, 1, knock_out=6, period=6)[0] == 4

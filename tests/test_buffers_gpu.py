"""The memory around a call (include/smfft.h, "Buffer contract"): every kernel against the bytes it must not write and the bytes it
must not read, at interior pointers and in place.

Every buffer is an allocation of its own laid out as [guard | payload | guard], 128 KiB of guard on each side: more than a whole tile
(32 KiB at most) or a FIR history of N - 1 samples, so even a wrong kernel touches only this test's memory.  The guards, the part of
an input a call must not read and the part of an output it must not write ([slots, nFFTs) of the `multiple` paths) hold a quiet NaN
with a payload of its own (0x7FE5A5A5); the part of the output the call must write is prefilled with 0xFF NaN.  After each call:
  1. the written output is within the suite's fp64 tolerances (oracle/np_reference.py; sqrt(k) for k applications);
  2. every other byte of the output allocation is unchanged (a stray write);
  3. the input allocation is unchanged, guards included (unless the call is in place);
  4. the output has the bits of the same call on exact-size buffers at an allocation base: results do not depend on where
     the buffers are.
A stray READ of a guard or of an unread part of the input brings the NaN payload into an output and fails 1.
Payloads sit 8 bytes past the front guard (the first FFT at an odd float2 index); the largest batch of each case also at 0 and
4096 - 8 bytes, once with a grid of one workgroup (the grid-stride loop reaches the ragged tile) and, on the `multiple` paths, once
with the balanced schedule cutting the chain of the last, partly filled tile (the parked store of lds_to_shared_tile is bounded by its
buffer descriptor alone)."""
import ctypes
import time

import numpy as np
import pytest

from oracle import np_reference as ref
from tests.fir_gpu_harness import _check_rows
from tests.fir_gpu_harness import _reference as _fir_reference
from tests.guarded_region import GUARD      # (128 KiB on each side of every payload, poisoned with a quiet NaN)
from tests.guarded_region import Region as _Region      # (offsets in whole float2: its default alignment)
from tests.guarded_region import poison as _poison

pytestmark = pytest.mark.gpu

UNWRITTEN = 0xFF               # NaN prefill of the bytes a call must write
OFFSET = 8                     # payload placement past the guard: an odd float2 index
MORE_OFFSETS = (0, 4096 - 8)   # and, for the largest batch of every case, these
REUSES = 3                     # applications per chain on the multiple paths (100 overflow fp32)
C2C_SIZES = [32, 64, 128, 256, 512, 1024, 2048, 4096]
R2C_SIZES = [512, 1024, 2048, 4096]


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    assert smfft_amd.lib.smfft_device_count() >= 1, "no HIP device"
    smfft_amd.FFT_init()
    return smfft_amd


# ------------------------------------------------------------------------------------------------------------- the guarded call
def _first_change(now, before, lo):
    idx = np.flatnonzero(now != before)
    return f"{len(idx)} bytes changed, the first at payload offset {int(idx[0]) - lo}" if len(idx) else ""


def _guarded(sm, call, x, total, out_fft_bytes, written, offset=OFFSET, in_place=False):
    """call(d_in, d_out) -> status on guarded buffers.  x: the FFTs the call reads (host array, one row per FFT); total: FFTs the
    caller's buffers hold (nFFTs; the input beyond x is poison, the call must not read it); written: output FFTs the call must write
    (the output beyond them is poison, the call must not write it).  Returns the written bytes (uint8)."""
    x = np.ascontiguousarray(x)
    in_fft_bytes = x.nbytes // x.shape[0]
    wb = written * out_fft_bytes
    inp = _poison(total * in_fft_bytes)
    inp[:x.nbytes] = x.view(np.uint8).reshape(-1)
    src = _Region(sm, inp, offset)
    if in_place:
        assert in_fft_bytes == out_fft_bytes and x.nbytes == wb
        dst = src
    else:
        out = _poison(total * out_fft_bytes)
        out[:wb] = UNWRITTEN
        dst = _Region(sm, out, offset)
    try:
        rc = call(src.ptr, dst.ptr)
        assert rc == 0, f"call returned {rc}"
        assert sm.lib.smfft_synchronize() == 0
        now = dst.read()
        lo = dst.lo
        before = dst.image
        what = _first_change(now[:lo], before[:lo], lo) or _first_change(now[lo + wb:], before[lo + wb:], -wb)
        assert not what, f"stray write outside the output FFTs [0, {written}): {what}"
        if not in_place:
            what = _first_change(src.read(), src.image, src.lo)
            assert not what, f"the input allocation changed: {what}"
        return now[lo:lo + wb].copy()
    finally:
        src.buf.free()
        if not in_place:
            dst.buf.free()


def _at_base(sm, call, x_full, out_dtype, out_shape):
    """the same call on exact-size buffers at an allocation base, as smfft_amd.api's conveniences make them"""
    din = sm.DeviceBuffer.from_host(np.ascontiguousarray(x_full))
    dout = sm.DeviceBuffer(int(np.prod(out_shape)) * np.dtype(out_dtype).itemsize)
    try:
        assert sm.lib.smfft_memset(dout.ptr, 0xFF, dout.nbytes) == 0
        assert call(din.ptr, dout.ptr) == 0
        assert sm.lib.smfft_synchronize() == 0
        return dout.to_host(out_dtype, out_shape)
    finally:
        din.free()
        dout.free()


def _same_bits(got, base, what):
    g, b = got.view(np.uint8), np.ascontiguousarray(base).view(np.uint8).reshape(-1)[:got.size]
    assert np.array_equal(g, b), f"{what}: the result depends on where the buffers are"


def _within(got, want, k, what):
    l2, mx = ref.fft_errors(got, want)
    assert l2 <= ref.REL_L2_TOL * k ** 0.5 and mx <= ref.MAX_ABS_TOL * k ** 0.5, f"{what}: relL2={l2:.3e} maxabs={mx:.3e} (k={k})"


class _Settings:
    """per-thread launch state changed inside a `with` block and restored on the way out"""

    def __init__(self, sm, nreuses=0, grid_cap=None, balance=None):
        self.sm, self.nreuses, self.grid_cap, self.balance = sm, nreuses, grid_cap, balance

    def __enter__(self):
        lib = self.sm.lib
        self.old_cap = lib.smfft_get_grid_cap()
        lib.smfft_set_nreuses(self.nreuses)
        if self.grid_cap is not None:
            lib.smfft_set_grid_cap(self.grid_cap)
        if self.balance is not None:
            lib.smfft_set_multiple_balance(self.balance)
        return self

    def __exit__(self, *exc):
        lib = self.sm.lib
        lib.smfft_set_nreuses(0)
        lib.smfft_set_grid_cap(self.old_cap)
        lib.smfft_set_multiple_balance(-1)
        lib.smfft_set_handoff_wait_us(-1)
        lib.smfft_debug_delay_parking(-1, 0, 0)
        return False


# ------------------------------------------------------------------------------------------------------------- the matrix
def _rand_c(rng, rows, n):
    return ((rng.random((rows, n), dtype=np.float32) - 0.5) + 1j * (rng.random((rows, n), dtype=np.float32) - 0.5)).astype(np.complex64)


def _batches(tile, unit=1):
    """1, T - 1, T + 1 and 3T + 1 FFTs for a tile of T (in slot units of `unit` on the N = 32 / 64 multiple paths), ascending"""
    return sorted({b for b in (unit, tile - unit, tile + unit, 3 * tile + unit) if b > 0})


def _cut_chains(ntiles, reuses, g):
    """chains a balanced launch over g workgroups cuts, with the application they are cut at (smfft_inst.hip, launch_compact; as
    tests/test_gpu_parity.py)"""
    total = ntiles * reuses
    per_wg = -(-total // g)
    return [(b // reuses, b % reuses) for b in range(per_wg, total, per_wg) if b % reuses]


def _ragged_cut(tile, unit):
    """(slots, g): 7 compact tiles, the last partly filled (when a tile holds more than one slot unit), and a number of workgroups
    whose balanced schedule cuts the last tile's chain"""
    ntiles = 7
    slots = ntiles * tile - (tile // 2 // unit * unit if tile > unit else 0)
    for g in range(2, ntiles):
        if any(c == ntiles - 1 for c, _ in _cut_chains(ntiles, REUSES, g)):
            return slots, g
    raise AssertionError("no balanced grid cuts the last chain")


class _Case:
    """One family / path / direction: how to launch it, its reference, its tile."""

    def __init__(self, family, path, n, inverse, reorder=True):
        self.family, self.path, self.n, self.inverse, self.reorder = family, path, n, inverse, reorder
        cn = n // 2 if family == "rc" else n                              # the complex length of the tile geometry
        if family == "dif":
            self.tile = 1024 // n if n <= 1024 else 1
        elif path == 0:
            self.tile = 4096 // cn
        else:
            self.tile = max(1, 1024 // cn)
        self.unit = (4 if n == 32 else 2 if n == 64 else 1) if (family == "ct" and path) else 1
        self.real_in = family == "rc" and not inverse
        self.real_out = family == "rc" and inverse

    def what(self):
        return f"{self.family} path={self.path} N={self.n} inverse={int(self.inverse)} reorder={int(self.reorder)}"

    def nffts(self, count):
        return count if self.path == 0 else 100 * count + 37

    def call(self, sm, nffts):
        if self.family == "dif":
            return lambda i, o: sm.lib.smfft_ct_dif_launch(i, o, self.n, nffts, int(self.inverse), None)
        fam = {"ct": 0, "st": 1, "rc": 2}[self.family]
        return lambda i, o: sm.lib.smfft_launch(fam, self.path, i, o, self.n, nffts, int(self.inverse), int(self.reorder), None)

    def input(self, rng, count):
        if self.real_in:
            return (rng.random((count, self.n), dtype=np.float32) - 0.5)
        return _rand_c(rng, count, self.n // 2 if self.real_out else self.n)

    def fft_bytes(self):
        return self.n * (4 if self.family == "rc" else 8)

    def reference(self, x, k):
        """k applications in fp64: R2C / C2R re-apply themselves to the previous output's bytes (RC:367-384)"""
        if self.family == "rc" and not self.inverse:
            y = np.asarray(x, np.float64)
            for _ in range(k):
                p = ref.r2c_packed(y)
                y = p.view(np.float64).reshape(len(x), self.n)
            return p
        if self.family == "rc":
            y = np.asarray(x, np.complex128)
            for _ in range(k):
                r = ref.c2r_packed(y)
                y = r.view(np.complex128).reshape(len(x), self.n // 2)
            return r
        y = x
        for _ in range(k):
            if self.family == "dif":
                y = ref.ct_c2c(y, self.inverse, True)[:, ref.bitrev_indices(self.n)]
            else:
                y = ref.ct_c2c(y, self.inverse, self.reorder)
        return y

    def result(self, raw, count):
        if self.real_out:
            return raw.view(np.float32).reshape(count, self.n)
        return raw.view(np.complex64).reshape(count, -1)

    def out_shape(self, nffts):
        return (nffts, self.n) if self.real_out else (nffts, self.n // 2 if self.family == "rc" else self.n)


def _run_case(sm, case, rng, count, offset=OFFSET, in_place=False, k=1):
    """one guarded call of `count` FFTs (slots on the multiple paths) checked against fp64 and against the same call at a base"""
    nffts = case.nffts(count)
    x = case.input(rng, count)
    raw = _guarded(sm, case.call(sm, nffts), x, nffts, case.fft_bytes(), count, offset, in_place)
    got = case.result(raw, count)
    what = f"{case.what()} count={count} nFFTs={nffts} offset={offset}{' in place' if in_place else ''}"
    _within(got, case.reference(x, k), k, what)
    x_full = np.zeros((nffts,) + x.shape[1:], x.dtype)
    x_full[:count] = x
    base = _at_base(sm, case.call(sm, nffts), x_full, np.float32 if case.real_out else np.complex64, case.out_shape(nffts))
    _same_bits(raw, base, what)


def _sweep(sm, case, seed):
    """every batch of the case at the standard offset; the largest also at the other offsets, under a one-workgroup grid, and (multiple
    paths) with the balanced schedule cutting the chain of the last, ragged tile"""
    rng = np.random.default_rng(seed)
    k = REUSES if case.path else 1
    with _Settings(sm, nreuses=REUSES if case.path else 0):
        batches = _batches(case.tile, case.unit)
        for count in batches:
            _run_case(sm, case, rng, count, k=k)
        for offset in MORE_OFFSETS:
            _run_case(sm, case, rng, batches[-1], offset=offset, k=k)
    with _Settings(sm, nreuses=REUSES if case.path else 0, grid_cap=1):
        _run_case(sm, case, rng, batches[-1], k=k)
    if case.path:
        slots, g = _ragged_cut(case.tile, case.unit)
        with _Settings(sm, nreuses=REUSES, balance=g):
            _run_case(sm, case, rng, slots, k=k)


@pytest.mark.parametrize("n", C2C_SIZES)
@pytest.mark.parametrize("inv,reo", [(0, 1), (0, 0), (1, 1), (1, 0)])
def test_ct_external_bounds(sm, n, inv, reo):
    _sweep(sm, _Case("ct", 0, n, bool(inv), bool(reo)), 100 * n + 10 * inv + reo)


@pytest.mark.parametrize("n", C2C_SIZES)
@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("inv,reo", [(0, 1), (0, 0), (1, 1), (1, 0)])
def test_ct_multiple_bounds(sm, n, path, inv, reo):
    _sweep(sm, _Case("ct", path, n, bool(inv), bool(reo)), 200 * n + 20 * path + 10 * inv + reo)


@pytest.mark.parametrize("n", C2C_SIZES)
@pytest.mark.parametrize("path", [0, 1, 2])
@pytest.mark.parametrize("inv", [1, 0])
def test_stockham_bounds(sm, n, path, inv):
    _sweep(sm, _Case("st", path, n, bool(inv)), 300 * n + 10 * path + inv)


@pytest.mark.parametrize("n", R2C_SIZES)
@pytest.mark.parametrize("path", [0, 1, 2])
@pytest.mark.parametrize("inv", [0, 1])
def test_rc_bounds(sm, n, path, inv):
    _sweep(sm, _Case("rc", path, n, bool(inv)), 400 * n + 10 * path + inv)


@pytest.mark.parametrize("n", C2C_SIZES)
@pytest.mark.parametrize("inv", [0, 1])
def test_dif_bounds(sm, n, inv):
    _sweep(sm, _Case("dif", 0, n, bool(inv), False), 500 * n + inv)


# ------------------------------------------------------------------------------------------------------------- in place
@pytest.mark.parametrize("n", [32, 1024, 4096])
@pytest.mark.parametrize("family", ["ct", "ct_noreorder", "st", "rc", "dif"])
@pytest.mark.parametrize("inv", [0, 1])
def test_in_place_external(sm, n, family, inv):
    """d_output == d_input for path 0 of every family and for the DIF transform: the largest batch of the case, one workgroup per tile
    and one workgroup for the whole batch"""
    if family == "rc" and n == 32:
        n = 512                                                    # (R2C / C2R start at 512)
    case = {"ct": _Case("ct", 0, n, bool(inv)), "ct_noreorder": _Case("ct", 0, n, bool(inv), False), "st": _Case("st", 0, n, bool(inv)),
            "rc": _Case("rc", 0, n, bool(inv)), "dif": _Case("dif", 0, n, bool(inv), False)}[family]
    rng = np.random.default_rng(600 * n + inv)
    count = _batches(case.tile)[-1]
    for cap in (0, 1):
        with _Settings(sm, grid_cap=cap):
            _run_case(sm, case, rng, count, in_place=True)


@pytest.mark.parametrize("family,n,inv,reo", [("ct", 32, 0, 1), ("ct", 64, 1, 0), ("ct", 256, 0, 0), ("ct", 1024, 1, 1),
                                              ("ct", 4096, 0, 1), ("st", 2048, 1, 1), ("rc", 1024, 0, 1), ("rc", 4096, 1, 1)])
@pytest.mark.parametrize("path", [1, 2])
def test_in_place_multiple_cut_chains(sm, family, n, inv, reo, path):
    """d_output == d_input on the multiple paths with chains cut by the balanced schedule: the parked data of a cut chain go to its own
    slot, which in place is also its input; the last, ragged tile's chain is one of those cut"""
    case = _Case(family, path, n, bool(inv), bool(reo))
    slots, g = _ragged_cut(case.tile, case.unit)
    with _Settings(sm, nreuses=REUSES, balance=g):
        _run_case(sm, case, np.random.default_rng(700 * n + path), slots, in_place=True, k=REUSES)


@pytest.mark.parametrize("after_commit", [0, 1])
def test_in_place_late_owner(sm, after_commit):
    """A balanced launch in place whose owner of a cut chain is held back 1.5 s (smfft_debug_delay_parking, as
    test_balanced_schedule_survives_a_late_owner): before its commit (0) the resumer takes the chain and reruns it from d_input -- which
    in place is the chain's output slot, still untouched -- and the late owner leaves it alone; after (1) the resumer waits for the
    parked data."""
    n, reuses, g, ntiles = 256, 7, 5, 23
    case = _Case("ct", 1, n, False)
    slots = ntiles * case.tile
    cuts = _cut_chains(ntiles, reuses, g)
    assert len(cuts) >= 3
    rng = np.random.default_rng(800 + after_commit)
    with _Settings(sm, nreuses=reuses, balance=g):
        sm.lib.smfft_set_handoff_wait_us(2000)
        sm.lib.smfft_debug_delay_parking(cuts[1][0], 1500, after_commit)
        t0 = time.time()
        nffts = case.nffts(slots)
        x = case.input(rng, slots)
        raw = _guarded(sm, case.call(sm, nffts), x, nffts, case.fft_bytes(), slots, in_place=True)
        assert time.time() - t0 > 1.4                               # the delay really happened
        sm.lib.smfft_debug_delay_parking(-1, 0, 0)
        _within(case.result(raw, slots), case.reference(x, reuses), reuses, f"late owner after_commit={after_commit} in place")
        sm.lib.smfft_set_multiple_balance(0)
        x_full = np.zeros((nffts, n), np.complex64)
        x_full[:slots] = x
        _same_bits(raw, _at_base(sm, case.call(sm, nffts), x_full, np.complex64, (nffts, n)), "late owner in place")


# ------------------------------------------------------------------------------------------------------------- benchmark forms
def test_benchmark_forms(sm):
    """one call of every *_benchmark entry point at one length, on guarded buffers"""
    n = 256
    t = ctypes.c_double(0.0)
    T = ctypes.byref(t)
    lib = sm.lib
    ct0, ct1, ct2 = _Case("ct", 0, n, False), _Case("ct", 1, n, True), _Case("ct", 2, n, False)
    st0, st1 = _Case("st", 0, n, True), _Case("st", 1, n, True)
    rc0f, rc0i, rc1 = _Case("rc", 0, 1024, False), _Case("rc", 0, 1024, True), _Case("rc", 1, 1024, False)
    dif = _Case("dif", 0, n, False, False)
    forms = [
        (ct0, 1, lambda i, o, m: lib.smfft_ct_external_benchmark(i, o, n, m, 0, 1, T)),
        (ct1, REUSES, lambda i, o, m: lib.smfft_ct_multiple_benchmark(i, o, n, m, 1, 1, T)),
        (ct2, REUSES, lambda i, o, m: lib.smfft_ct_multiple_unfused_benchmark(i, o, n, m, 0, T)),
        (ct2, REUSES, lambda i, o, m: lib.smfft_ct_multiple_percall_benchmark(i, o, n, m, 0, 1, T)),
        (st0, 1, lambda i, o, m: lib.smfft_st_external_benchmark(i, o, n, m, T)),
        (_Case("st", 0, n, False), 1, lambda i, o, m: lib.smfft_st_external_benchmark_dir(i, o, n, m, 0, T)),
        (st1, REUSES, lambda i, o, m: lib.smfft_st_multiple_benchmark(i, o, n, m, T)),
        (rc0f, 1, lambda i, o, m: lib.smfft_rc_external_benchmark(i, o, 1024, m, 0, T)),
        (rc0i, 1, lambda i, o, m: lib.smfft_rc_external_benchmark(i, o, 1024, m, 1, T)),
        (rc1, REUSES, lambda i, o, m: lib.smfft_rc_multiple_benchmark(i, o, 1024, m, T)),
        (dif, 1, lambda i, o, m: lib.smfft_ct_dif_external_benchmark(i, o, n, m, 0, T)),
    ]
    rng = np.random.default_rng(900)
    with _Settings(sm, nreuses=REUSES):
        for case, k, form in forms:
            count = _batches(case.tile, case.unit)[-1]
            nffts = case.nffts(count)
            x = case.input(rng, count)
            raw = _guarded(sm, lambda i, o: form(i, o, nffts), x, nffts, case.fft_bytes(), count)
            _within(case.result(raw, count), case.reference(x, k), k, f"benchmark form of {case.what()}")
    # the FIR benchmark form
    N, M, C, K, L = 1024, 257, 3, 5, 2000
    x, h = _rand_c(rng, C, L), _rand_c(rng, K, M)
    spec = _fir_spectra_at_base(sm, h, N, "convolve")
    raw = _fir_guarded(sm, x, h, N, "convolve", spectra=spec, launch=lambda dx, ds, do: lib.smfft_fir_benchmark(dx, L, C, ds, K, M, N, 0, do, T))
    _check_rows(raw.view(np.complex64).reshape(C, K, L), _fir_reference(x, h, False), "smfft_fir_benchmark", x, h)


# ------------------------------------------------------------------------------------------------------------- FIR
def _fir_spectra_at_base(sm, h, N, mode):
    K, M = h.shape
    dh, ds = sm.DeviceBuffer.from_host(h), sm.DeviceBuffer(K * N * 8)
    try:
        sm.fir_prepare(dh.ptr, ds.ptr, M, K, N, mode)
        assert sm.lib.smfft_synchronize() == 0
        return ds.to_host(np.complex64, (K, N))
    finally:
        dh.free()
        ds.free()


def _fir_guarded(sm, x, h, N, mode, spectra=None, launch=None, offset=OFFSET):
    """spectra None: smfft_fir_prepare alone, returns the spectra's bytes; else `launch` (default smfft_fir_launch) with those spectra,
    returns the output's bytes.  Signal, taps, spectra and output are guarded allocations of their own, all checked after the call."""
    C, L = x.shape
    K, M = h.shape
    corr = 1 if mode == "correlate" else 0
    sig = _Region(sm, x.view(np.uint8).reshape(-1), offset)
    taps = _Region(sm, h.view(np.uint8).reshape(-1), offset)
    spec_bytes = spectra.view(np.uint8).reshape(-1) if spectra is not None else np.full(K * N * 8, UNWRITTEN, np.uint8)
    spec = _Region(sm, spec_bytes, offset)
    out = _Region(sm, np.full(C * K * L * 8, UNWRITTEN, np.uint8), offset)
    regions = (sig, taps, spec, out)
    try:
        if spectra is None:
            assert sm.lib.smfft_fir_prepare(taps.ptr, M, K, N, corr, spec.ptr, None) == 0
            assert sm.lib.smfft_synchronize() == 0
            now = spec.read()
            lo, nb = spec.lo, K * N * 8
            what = _first_change(now[:lo], spec.image[:lo], lo) or _first_change(now[lo + nb:], spec.image[lo + nb:], -nb)
            assert not what, f"prepare wrote outside spectra[0, K N): {what}"
            for r, name in ((sig, "signal"), (taps, "taps"), (out, "output")):
                what = _first_change(r.read(), r.image, r.lo)
                assert not what, f"prepare changed the {name} allocation: {what}"
            return now[lo:lo + nb].copy()
        if launch is None:
            launch = lambda dx, ds, do: sm.lib.smfft_fir_launch(dx, L, C, ds, K, M, N, corr, do, None)  # noqa: E731
        assert launch(sig.ptr, spec.ptr, out.ptr) == 0
        assert sm.lib.smfft_synchronize() == 0
        now = out.read()
        lo, nb = out.lo, C * K * L * 8
        what = _first_change(now[:lo], out.image[:lo], lo) or _first_change(now[lo + nb:], out.image[lo + nb:], -nb)
        assert not what, f"launch wrote outside out[0, C K L): {what}"
        for r, name in ((sig, "signal"), (taps, "taps"), (spec, "spectra")):
            what = _first_change(r.read(), r.image, r.lo)
            assert not what, f"the {name} allocation changed: {what}"
        return now[lo:lo + nb].copy()
    finally:
        for r in regions:
            r.buf.free()


# N = 256 / 1024 / 4096 with M = 1, N/4 + 1, N - 1; N = 512 / 2048 (their kernels) with the two extreme tap counts
FIR_CASES = [(N, r) for N in (256, 1024, 4096) for r in ("1", "N/4+1", "N-1")] + [(N, r) for N in (512, 2048) for r in ("1", "N-1")]


@pytest.mark.parametrize("N,M_rule", FIR_CASES)
@pytest.mark.parametrize("mode", ["convolve", "correlate"])
def test_fir_bounds(sm, N, M_rule, mode):
    """prepare and launch separately on guarded buffers: signal lengths below M, of one segment and of several with a ragged last one,
    1 and 3 channels, 1 and 5 filters.  The guard in front of channel 0 is what a convolution's history would read, the one behind
    channel C - 1 what a correlation's look-ahead would read; both must come in as zeros, never as the guard's NaN."""
    M = {"1": 1, "N/4+1": N // 4 + 1, "N-1": N - 1}[M_rule]
    V = N - M + 1
    rng = np.random.default_rng(N + 7 * M + (mode == "correlate"))
    for L in (max(1, M - 1) if M > 1 else 1, V, 2 * V + V // 3 + 1):
        for C, K in ((1, 1), (3, 5)):
            x, h = _rand_c(rng, C, L), _rand_c(rng, K, M)
            what = f"N={N} {mode} M={M} L={L} C={C} K={K}"
            spec = _fir_guarded(sm, x, h, N, mode).view(np.complex64).reshape(K, N)
            assert np.array_equal(spec.view(np.uint32), _fir_spectra_at_base(sm, h, N, mode).view(np.uint32)), f"{what}: spectra depend on placement"
            raw = _fir_guarded(sm, x, h, N, mode, spectra=spec)
            got = raw.view(np.complex64).reshape(C, K, L)
            _check_rows(got, _fir_reference(x, h, mode == "correlate"), what, x, h)
            assert np.array_equal(got.view(np.uint32), sm.fir(x, h, mode, fft_size=N).view(np.uint32)), f"{what}: result depends on placement"


# ------------------------------------------------------------------------------------------------------------- host transforms
def _host_block(sm, nbytes_in, nbytes_out, pinned):
    """one host block [guard | 8 | in | guard | 8 | out | guard] (pinned: smfft_host_malloc; else a pageable NumPy array), poisoned"""
    total = 3 * GUARD + 16 + nbytes_in + nbytes_out
    block = sm.pinned_empty((total,), np.uint8) if pinned else np.empty(total, np.uint8)
    block[:] = _poison(total)
    i0 = GUARD + 8
    o0 = i0 + nbytes_in + GUARD + 8
    return block, i0, o0


@pytest.mark.parametrize("n", [64, 1024])
@pytest.mark.parametrize("config", ["zero_copy", "slabs", "pageable"])
def test_host_transform_bounds(sm, n, config, monkeypatch):
    """smfft_host_transform at interior pointers of one guarded host block, with a ragged last slab: pinned memory through the kernel
    on host memory (zero copy) and through the slab pipeline (SMFFT_HOST_ZERO_COPY=0), and views into a larger pageable array"""
    if config == "slabs":
        monkeypatch.setenv("SMFFT_HOST_ZERO_COPY", "0")
    tile = 4096 // n
    nffts, slab = 5 * tile + 3, 2 * tile + 1
    x = _rand_c(np.random.default_rng(1000 + n), nffts, n)
    block, i0, o0 = _host_block(sm, x.nbytes, x.nbytes, config != "pageable")
    vin = block[i0:i0 + x.nbytes].view(np.complex64).reshape(nffts, n)
    vout = block[o0:o0 + x.nbytes].view(np.complex64).reshape(nffts, n)
    vin[...] = x
    vout.view(np.uint8)[...] = UNWRITTEN
    before = block.copy()
    t = ctypes.c_double(0.0)
    assert sm.lib.smfft_host_transform(0, vin.ctypes.data, vout.ctypes.data, n, nffts, 0, 1, slab, 2, ctypes.byref(t)) == 0
    now = block.copy()
    what = _first_change(np.r_[now[:o0], now[o0 + x.nbytes:]], np.r_[before[:o0], before[o0 + x.nbytes:]], 0)
    assert not what, f"host transform N={n} {config}: bytes outside the output changed: {what}"
    got = now[o0:o0 + x.nbytes].view(np.complex64).reshape(nffts, n)
    ref.assert_close_fp32(got, ref.ct_c2c(x, False, True), f"host transform N={n} {config}")
    _same_bits(got.view(np.uint8).reshape(-1), sm.c2c(x), f"host transform N={n} {config}")


@pytest.mark.parametrize("config", ["zero_copy", "slabs", "pageable"])
def test_host_transform_in_place(sm, config, monkeypatch):
    """h_output == h_input inside a guarded host block, each way through the host transform, with a ragged last slab"""
    if config == "slabs":
        monkeypatch.setenv("SMFFT_HOST_ZERO_COPY", "0")
    n, nffts = 1024, 11
    x = _rand_c(np.random.default_rng(1100), nffts, n)
    block, i0, _ = _host_block(sm, x.nbytes, 0, config != "pageable")
    v = block[i0:i0 + x.nbytes].view(np.complex64).reshape(nffts, n)
    v[...] = x
    before = block.copy()
    t = ctypes.c_double(0.0)
    assert sm.lib.smfft_host_transform(0, v.ctypes.data, v.ctypes.data, n, nffts, 1, 0, 4, 2, ctypes.byref(t)) == 0
    now = block.copy()
    what = _first_change(np.r_[now[:i0], now[i0 + x.nbytes:]], np.r_[before[:i0], before[i0 + x.nbytes:]], 0)
    assert not what, f"in-place host transform ({config}): bytes outside the buffer changed: {what}"
    got = now[i0:i0 + x.nbytes].view(np.complex64).reshape(nffts, n)
    ref.assert_close_fp32(got, ref.ct_c2c(x, True, False), f"in-place host transform ({config})")
    _same_bits(got.view(np.uint8).reshape(-1), sm.c2c(x, True, False), f"in-place host transform ({config})")

"""The per-call form of the in-LDS C2C path (smfft_launch path 2: SMFFT_DIT_multiple_unfused, one image load and one image store
per application), the Stockham-family and R2C-family `multiple` launches that no benchmark entry point reaches, and the two per-call
benchmark entry points -- against fp64 and against the fused kernels of path 1.

Every kernel path 2 ships is run in both directions: the natural-order transforms at N = 32 ... 4096 and the no-reorder lane engines
of N = 32 and 64.  The lane engines flip sign BITS in their load / store where a piece of a chain starts or ends on an odd
application (smfft_engine.hpp, PairEngine32 / QuadEngine64), so every check runs odd and even application counts, and the balanced
schedule cuts chains at odd and even applications.

Tolerances (fp32 data against the fp64 oracle, per FFT): relL2 <= 5e-7 * sqrt(k) and max|err| <= 1e-6 * sqrt(k) * max|ref| after k
applications -- the library's per-FFT bounds (oracle/np_reference.py) grown as independent roundings do.  Inputs are zero-mean: with
U[0, 1) data the DC bin dominates both norms and hides errors in the others.  Outputs are prefilled with NaN (0xFF) and every word
past the written slots must still be 0xFFFFFFFF."""
import ctypes

import numpy as np
import pytest

from oracle import np_reference as ref
from tests import oracle_api as oa

pytestmark = pytest.mark.gpu

C2C_SIZES = [32, 64, 128, 256, 512, 1024, 2048, 4096]
R2C_SIZES = [512, 1024, 2048, 4096]
NREUSES = 100
# the kernels path 2 has of its own (everything else on path 2 is the path-1 kernel): (N, reorder)
PERCALL_KERNELS = [(n, 1) for n in C2C_SIZES] + [(32, 0), (64, 0)]


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    assert smfft_amd.lib.smfft_device_count() >= 1, "no HIP device"
    smfft_amd.FFT_init()
    return smfft_amd


def _lane_engine(n, reo):
    return n == 32 or (n == 64 and not reo)


def _slot_unit(n):
    """the multiple path's slots come in groups of 4 (N = 32) / 2 (N = 64) FFTs (smfft_api.hip, ct_multiple_slots)"""
    return 4 if n == 32 else 2 if n == 64 else 1


def _batch(n, ntiles):
    """(slots, nFFTs): `ntiles` compact tiles of max(1, 1024 / N) FFTs with a ragged last tile, and nFFTs = 100 * slots + 37 (the
    remainder is not a slot)"""
    tile = max(1, 1024 // n)
    unit = _slot_unit(n)
    slots = ntiles * tile - (tile // 2 // unit * unit if tile > 1 else 0)
    nffts = NREUSES * slots + 37
    assert nffts // (NREUSES * unit) * unit == slots
    return slots, nffts


def _zero_mean(rng, shape, scale=1.0):
    x = (rng.random(shape, dtype=np.float32) - 0.5) + 1j * (rng.random(shape, dtype=np.float32) - 0.5)
    return (x * scale).astype(np.complex64)


def _launch(sm, family, path, x, n, nffts, inverse, reorder, out_dtype=np.complex64, out_shape=None):
    """smfft_launch on device copies of x into a NaN-prefilled output of the same bytes; returns the whole output"""
    din = sm.DeviceBuffer.from_host(x)
    dout = sm.DeviceBuffer(x.nbytes)
    assert sm.lib.smfft_memset(dout.ptr, 0xFF, x.nbytes) == 0
    sm.launch(family, path, din.ptr, dout.ptr, n, nffts, inverse=bool(inverse), reorder=bool(reorder))
    assert sm.lib.smfft_synchronize() == 0
    out = dout.to_host(out_dtype, x.shape if out_shape is None else out_shape)
    din.free()
    dout.free()
    return out


def _ct(sm, path, x, inv, reo):
    nffts, n = x.shape
    return _launch(sm, "ct", {1: "multiple", 2: "multiple_unfused"}[path], x, n, nffts, inv, reo)


def _chain(oracle_lib, x, inv, reo, k):
    want = x.astype(np.complex128)
    for _ in range(k):
        want = oa.ct_c2c(oracle_lib, want, inv, reo, "f64")
    return want


def _untouched(a):
    return bool((a.view(np.uint32) == 0xFFFFFFFF).all())


def _within(got, want, k, what):
    l2, mx = ref.fft_errors(got, want)
    assert l2 <= 5e-7 * k ** 0.5 and mx <= 1e-6 * k ** 0.5, f"{what}: relL2={l2:.3e} maxabs={mx:.3e} (k={k})"


# ------------------------------------------------------------------------------------ path 2 against fp64 and against path 1
@pytest.mark.parametrize("n", C2C_SIZES)
@pytest.mark.parametrize("inv", [0, 1])
@pytest.mark.parametrize("reo", [1, 0])
def test_percall_path_against_fp64_and_path1(sm, oracle_lib, n, inv, reo):
    """smfft_launch(0, 2, ...) after k = 1 ... 4 applications: k applications of the fp64 oracle; and its relation to path 1
    (include/smfft.h, smfft_ct_multiple_percall_benchmark): the lane engines (N = 32, N = 64 without reorder) give
    the fused loop's bits, the planar no-reorder kernels (N >= 128) ARE the path-1 kernels, the natural-order planar kernels agree to
    rounding (another instantiation: hipcc contracts a few multiply-adds differently)."""
    slots, nffts = _batch(n, 5)
    rng = np.random.default_rng(200 * n + 10 * inv + reo)
    x = _zero_mean(rng, (nffts, n))
    want = x[:slots].astype(np.complex128)
    try:
        for k in (1, 2, 3, 4):
            sm.lib.smfft_set_nreuses(k)
            percall = _ct(sm, 2, x, inv, reo)
            fused = _ct(sm, 1, x, inv, reo)
            assert _untouched(percall[slots:]), f"path 2 wrote past its {slots} slots (k={k})"
            want = oa.ct_c2c(oracle_lib, want, inv, reo, "f64")
            _within(percall[:slots], want, k, f"path 2 N={n} inv={inv} reo={reo}")
            if _lane_engine(n, reo) or not reo:
                assert np.array_equal(percall.view(np.uint32), fused.view(np.uint32)), (n, inv, reo, k)
            else:
                l2, mx = ref.fft_errors(percall[:slots], fused[:slots].astype(np.complex128))
                assert l2 < 5e-7 and mx < 2e-6, (n, inv, k, l2, mx)
    finally:
        sm.lib.smfft_set_nreuses(0)


@pytest.mark.parametrize("n,reo", PERCALL_KERNELS)
@pytest.mark.parametrize("inv", [0, 1])
def test_percall_balanced_schedule_is_bit_identical(sm, oracle_lib, n, reo, inv):
    """Path 2 on the balanced schedule (a cut chain is parked in its output slot and resumed by another workgroup: the FUSED = false
    bodies' shared_tile_to_lds / shared_tile_to_planes) over 2, 3 and 7 workgroups at 3, 4 and 7 applications gives the bits of one
    chain per workgroup -- chains cut at odd and even applications, ragged last tile included -- and those bits are k applications of
    the fp64 oracle (a fault that every schedule shares is no difference between them)."""
    ntiles = 23
    slots, nffts = _batch(n, ntiles)
    rng = np.random.default_rng(4100 + n + 2 * inv + reo)
    x = _zero_mean(rng, (nffts, n))
    cut_parity = set()
    try:
        for reuses in (3, 4, 7):
            sm.lib.smfft_set_nreuses(reuses)
            sm.lib.smfft_set_multiple_balance(0)
            want = _ct(sm, 2, x, inv, reo)
            assert _untouched(want[slots:])
            _within(want[:slots], _chain(oracle_lib, x[:slots], inv, reo, reuses), reuses, f"path 2 N={n} inv={inv} reo={reo}")
            for g in (2, 3, 7):
                sm.lib.smfft_set_multiple_balance(g)
                got = _ct(sm, 2, x, inv, reo)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, reo, inv, reuses, g)
                total = ntiles * reuses
                per_wg = -(-total // g)
                cut_parity |= {b % reuses % 2 for b in range(per_wg, total, per_wg) if b % reuses}
    finally:
        sm.lib.smfft_set_nreuses(0)
        sm.lib.smfft_set_multiple_balance(-1)
    assert cut_parity == {0, 1}


@pytest.mark.parametrize("n,reo", [(32, 1), (32, 0), (64, 0)])
@pytest.mark.parametrize("inv", [0, 1])
@pytest.mark.parametrize("reuses", [39, 40])
def test_percall_long_chains_against_the_oracle(sm, oracle_lib, n, reo, inv, reuses):
    """39 and 40 applications on path 2 (data scaled by 2^-100 so that N^(k/2) stays finite in fp32), on the product schedule, against
    k applications of the fp64 oracle: the lane engines end odd and even chains in different sign states."""
    tile = max(1, 1024 // n)
    nffts = (61 * tile - tile // 2) * NREUSES
    slots = nffts // (NREUSES * _slot_unit(n)) * _slot_unit(n)
    rng = np.random.default_rng(7100 + n + reuses + 2 * inv + reo)
    x = _zero_mean(rng, (nffts, n), np.ldexp(np.float32(1), -100))
    sm.lib.smfft_set_nreuses(reuses)
    try:
        got = _ct(sm, 2, x, inv, reo)
    finally:
        sm.lib.smfft_set_nreuses(0)
    assert _untouched(got[slots:])
    assert np.isfinite(got[:slots].view(np.float32)).all()
    _within(got[:slots], _chain(oracle_lib, x[:slots], inv, reo, reuses), reuses, f"path 2 N={n} inv={inv} reo={reo}")


# ------------------------------------------------------------------------------------------- the per-call benchmark entry points
def _benchmark(sm, fn, x, n, nffts, *args):
    """(status, *FFT_time starting at 1.0, output) of one benchmark call into a NaN-prefilled output"""
    din = sm.DeviceBuffer.from_host(x)
    dout = sm.DeviceBuffer(x.nbytes)
    assert sm.lib.smfft_memset(dout.ptr, 0xFF, x.nbytes) == 0
    t = ctypes.c_double(1.0)
    rc = fn(din.ptr, dout.ptr, n, nffts, *args, ctypes.byref(t))
    assert sm.lib.smfft_synchronize() == 0
    out = dout.to_host(np.complex64, x.shape)
    din.free()
    dout.free()
    return rc, t.value, out


@pytest.mark.parametrize("n", [32, 64, 1024])
def test_percall_benchmark_entry_points(sm, n):
    """smfft_ct_multiple_percall_benchmark (both directions and orders) and smfft_ct_multiple_unfused_benchmark (natural order): status 0,
    the elapsed time ADDED to *FFT_time, and the bits of smfft_launch path 2 at the same application count; with fewer than 100 FFTs
    status 1, *FFT_time = -1 and nothing written; an unsupported length writes nothing."""
    slots, nffts = _batch(n, 3)
    rng = np.random.default_rng(9000 + n)
    x = _zero_mean(rng, (nffts, n))
    sm.lib.smfft_set_nreuses(3)
    try:
        for inv in (0, 1):
            for reo in (1, 0):
                want = _ct(sm, 2, x, inv, reo)
                assert np.isfinite(want[:slots].view(np.float32)).all() and _untouched(want[slots:])
                rc, t, got = _benchmark(sm, sm.lib.smfft_ct_multiple_percall_benchmark, x, n, nffts, inv, reo)
                assert rc == 0 and t > 1.0, (inv, reo, rc, t)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ("percall", inv, reo)
                if reo:
                    rc, t, got = _benchmark(sm, sm.lib.smfft_ct_multiple_unfused_benchmark, x, n, nffts, inv)
                    assert rc == 0 and t > 1.0, (inv, rc, t)
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ("unfused", inv)
        small = x[:99]
        for fn, args in ((sm.lib.smfft_ct_multiple_percall_benchmark, (0, 1)), (sm.lib.smfft_ct_multiple_percall_benchmark, (1, 0)),
                         (sm.lib.smfft_ct_multiple_unfused_benchmark, (1,))):
            rc, t, got = _benchmark(sm, fn, small, n, 99, *args)
            assert rc == 1 and t == -1.0, (args, rc, t)
            assert _untouched(got)
    finally:
        sm.lib.smfft_set_nreuses(0)


def test_percall_benchmark_unsupported_length(sm):
    """N = 48: status 0 ("Error wrong FFT length!", as every benchmark entry point), nothing written"""
    x = _zero_mean(np.random.default_rng(48), (400, 48))
    for fn, args in ((sm.lib.smfft_ct_multiple_percall_benchmark, (0, 1)), (sm.lib.smfft_ct_multiple_percall_benchmark, (1, 0)),
                     (sm.lib.smfft_ct_multiple_unfused_benchmark, (0,))):
        rc, t, got = _benchmark(sm, fn, x, 48, 400, *args)
        assert rc == 0, (args, rc)
        assert _untouched(got)


# ------------------------------------------------------------------- the Stockham and R2C families' `multiple` launches
@pytest.mark.parametrize("n", C2C_SIZES)
@pytest.mark.parametrize("path", [1, 2])
def test_stockham_forward_multiple_launch(sm, oracle_lib, n, path):
    """smfft_launch(1, path, inverse = 0) is the forward extension on the CT natural-order kernels over nFFTs / 100 slots -- NOT rounded
    to the pairs / quads of ct_multiple_slots: 37 slots end in a partial quad (N = 32) and pair (N = 64).  k = 1, 2, 3 forward DFTs."""
    slots = 37
    nffts = NREUSES * slots + 5
    rng = np.random.default_rng(3700 + n + path)
    x = _zero_mean(rng, (nffts, n))
    want = x[:slots].astype(np.complex128)
    try:
        for k in (1, 2, 3):
            sm.lib.smfft_set_nreuses(k)
            got = _launch(sm, "st", {1: "multiple", 2: "multiple_unfused"}[path], x, n, nffts, False, True)
            want = oa.ct_c2c(oracle_lib, want, 0, 1, "f64")
            assert _untouched(got[slots:]), f"wrote past {slots} slots (k={k})"
            _within(got[:slots], want, k, f"ST forward multiple N={n} path={path}")
    finally:
        sm.lib.smfft_set_nreuses(0)


@pytest.mark.parametrize("n", C2C_SIZES)
def test_stockham_inverse_path2_is_path1(sm, n):
    """smfft_launch(1, 2, inverse = 1) runs the path-1 Stockham kernel: the same bits"""
    slots = 37
    nffts = NREUSES * slots + 5
    x = _zero_mean(np.random.default_rng(3800 + n), (nffts, n))
    sm.lib.smfft_set_nreuses(3)
    try:
        p1 = _launch(sm, "st", "multiple", x, n, nffts, True, True)
        p2 = _launch(sm, "st", "multiple_unfused", x, n, nffts, True, True)
    finally:
        sm.lib.smfft_set_nreuses(0)
    assert np.isfinite(p1[:slots].view(np.float32)).all() and _untouched(p1[slots:])
    assert np.array_equal(p1.view(np.uint32), p2.view(np.uint32))


@pytest.mark.parametrize("n", R2C_SIZES)
@pytest.mark.parametrize("inv", [0, 1])
def test_r2c_family_path2_is_path1(sm, n, inv):
    """smfft_launch(2, 2, ...) runs the path-1 R2C / C2R kernels: the same bits"""
    slots = 37
    nffts = NREUSES * slots + 5
    rng = np.random.default_rng(3900 + n + inv)
    if inv:
        x, shape, dt = _zero_mean(rng, (nffts, n // 2)), (nffts, n), np.float32
    else:
        x, shape, dt = rng.random((nffts, n), dtype=np.float32) - np.float32(0.5), (nffts, n // 2), np.complex64
    sm.lib.smfft_set_nreuses(3)
    try:
        p1 = _launch(sm, "rc", "multiple", x, n, nffts, inv, True, dt, shape)
        p2 = _launch(sm, "rc", "multiple_unfused", x, n, nffts, inv, True, dt, shape)
    finally:
        sm.lib.smfft_set_nreuses(0)
    assert np.isfinite(p1[:slots].view(np.float32)).all() and _untouched(p1[slots:])
    assert np.array_equal(p1.view(np.uint32), p2.view(np.uint32))


@pytest.mark.parametrize("n", R2C_SIZES)
@pytest.mark.parametrize("reuses", [2, 3])
def test_c2r_multiple_chains(sm, n, reuses):
    """The C2R `multiple` launch re-applies the C2R in LDS: the N reals of one application are the N / 2 packed complex values of the
    next.  k = 2, 3 applications of np_reference.c2r_packed in fp64."""
    nffts = NREUSES * (4096 // (n // 2) + 3) + 41
    slots = nffts // NREUSES
    xp = _zero_mean(np.random.default_rng(5000 + n + reuses), (nffts, n // 2))
    sm.lib.smfft_set_nreuses(reuses)
    try:
        got = _launch(sm, "rc", "multiple", xp, n, nffts, True, True, np.float32, (nffts, n))
    finally:
        sm.lib.smfft_set_nreuses(0)
    assert _untouched(got[slots:])
    want = xp[:slots].astype(np.complex128)
    for k in range(reuses):
        real = ref.c2r_packed(want)
        want = real.view(np.complex128).reshape(slots, n // 2)
    _within(got[:slots], real, reuses, f"C2R multiple N={n} x{reuses}")

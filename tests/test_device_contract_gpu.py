"""The header-only device API (include/smfft_device.hpp) beyond do_SMFFT_CT_DIT: user kernels around do_FFT_Stockham_mk6,
do_FFT_Stockham_C2C, do_FFT_Stockham_R2C_C2R, the registers forms, the smfft::tiled functions, FFT_GPU_external at N = 32 ... 128
and the header's `multiple` kernels, each compared with numpy complex128 by the conventions S1 / S3 ... S6 of DESIGN.md section 1
(oracle/np_reference.py).  The kernels are tests/hip/device_contract.hip, built by smfft_amd/csrc/Makefile in four builds of the
header (BUILDS) and a -DNREUSES=3 build for the `multiple` kernels.

Every case prefills its output with 0xFF (NaN), so an element that is never written fails; runs a ragged number of blocks (37); and
for the fill / call / drain, registers and tiled kernels also runs with the function's documented LDS footprint plus 64 float2 whose
contents must come out unchanged (a write past the footprint would otherwise land in other LDS unseen).  Tolerances are
oracle/np_reference.py's per-FFT relL2 <= 5e-7, max|err| <= 1e-6 * max|ref|, times sqrt(k) for chains of k applications, as in
tests/test_gpu_parity.py."""
import ctypes
import os

import numpy as np
import pytest

from oracle import np_reference as ref

pytestmark = pytest.mark.gpu

SIZES = [32, 64, 128, 256, 512, 1024, 2048, 4096]
R2C_L = [32, 64, 128, 256, 512, 1024, 2048]       # complex length L = real length / 2 (the library's R2C API: L = 256 ... 2048)
BUILDS = ["", "_unfused_io", "_no_phases", "_no_pairs"]
BLOCKS = 37
ST_FNS = {0: "mk6", 1: "C2C forward", 2: "C2C inverse", 3: "R2C", 4: "C2R"}

_VP, _I = ctypes.c_void_p, ctypes.c_int
_ARGTYPES = {
    "dc_stockham": [_I, _VP, _VP, _I, _I, _VP, _VP],
    "dc_chain": [_I, _VP, _VP, _I, _I, _I, _VP],
    "dc_tiled": [_I, _VP, _VP, _I, _I, _VP, _VP],
    "dc_tiled_ct": [_I, _I, _VP, _VP, _I, _I, _VP, _VP],
    "dc_stockham_registers": [_I, _I, _VP, _VP, _I, _I, _VP, _VP],
    "dc_ct_registers": [_I, _I, _VP, _VP, _I, _I, _VP, _VP],
    "dc_fft_gpu_external": [_VP, _VP, _I, _I, _VP],
    "dc_ct_multiple": [_I, _I, _I, _VP, _VP, _I, _I, _VP],
    "dc_fft_gpu_multiple": [_VP, _VP, _I, _I, _VP],
    "dc_rc_multiple": [_I, _VP, _VP, _I, _I, _VP],
    "dc_nreuses": [],
}


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    assert smfft_amd.lib.smfft_device_count() >= 1, "no HIP device"
    smfft_amd.FFT_init()
    return smfft_amd


_LIBS = {}


def _lib(sm, build=""):
    if build not in _LIBS:
        path = os.path.join(os.path.dirname(sm.LIB_PATH), f"libsmfft_device_contract{build}.so")
        if not os.path.exists(path):
            pytest.fail(f"libsmfft_device_contract{build}.so is missing: it is built by smfft_amd/csrc/Makefile -- a GPU run without it is a broken build, not a skip")
        lib = ctypes.CDLL(path)
        for name, args in _ARGTYPES.items():
            getattr(lib, name).argtypes = args
        _LIBS[build] = lib
    return _LIBS[build]


def _complex(rng, shape):
    return ((rng.random(shape, dtype=np.float32) - 0.5) + 1j * (rng.random(shape, dtype=np.float32) - 0.5)).astype(np.complex64)


def _launch(sm, call, x, out_dtype, out_shape, canary=False):
    """call(in_ptr, out_ptr, canary_ptr) -> status; returns the output (prefilled with NaN) and the canary count"""
    din = sm.DeviceBuffer.from_host(x)
    dout = sm.DeviceBuffer(x.nbytes)
    sm.lib.smfft_memset(dout.ptr, 0xFF, x.nbytes)
    dcan = None
    if canary:
        dcan = sm.DeviceBuffer(8)
        sm.lib.smfft_memset(dcan.ptr, 0, 8)
    assert call(din.ptr, dout.ptr, dcan.ptr if canary else None) == 0
    assert sm.lib.smfft_synchronize() == 0
    got = dout.to_host(out_dtype, out_shape)
    changed = int(dcan.to_host(np.int32, (1,))[0]) if canary else 0
    for b in (din, dout, dcan):
        if b is not None:
            b.free()
    return got, changed


def _want(fn, n, x):
    """fp64 result of the Stockham-family function fn (ST_FNS) on x: complex (nFFTs, N), or for C2R the reals (nFFTs, 2L)"""
    if fn == 0:
        return ref.st_c2c(x, inverse=True)
    if fn in (1, 2):
        return ref.st_c2c(x, inverse=fn == 2)
    if fn == 3:
        return ref.r2c_packed(x.view(np.float32).reshape(x.shape[0], 2 * n))
    return ref.c2r_packed(x)


def _check(fn, got, want, what):
    """got: the kernel's complex64 output; C2R (fn 4) compares it as the reals it holds"""
    if fn == 4:
        got = got.view(np.float32).reshape(want.shape)
    ref.assert_close_fp32(got, want, what)


def _check_both_footprints(sm, fn, call, x, want, what):
    """the footprint plus the canary words (first: a write past the footprint is reported as such) and the exact footprint: no canary
    word changed, the fp64 result both times"""
    for canary in (True, False):
        got, changed = _launch(sm, call, x, np.complex64, x.shape, canary)
        assert changed == 0, f"{what}: {changed} LDS words past the documented footprint changed"
        _check(fn, got, want, f"{what} canary={canary}")


# ------------------------------------------------------------------ fill / call / drain, reference shape
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("fn", [0, 1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_stockham_fill_call_drain(sm, n, fn, build):
    """<<<37, N/4>>>: fill s, barrier, do_FFT_Stockham_mk6<FFT_N>(s) on exactly N float2 of dynamic LDS (ST:309-319) or
    do_FFT_Stockham_C2C<FFT_N, D>(s) on N + 1 (RC), and drain right after the call with no barrier of the caller's: the function's
    own trailing barrier is what orders it (ST:253, RC:360-361).  mk6 is the + sign transform (S3), C2C the transform of its
    direction (S4), both natural order."""
    lib = _lib(sm, build)
    x = _complex(np.random.default_rng(100 * n + fn), (BLOCKS, n))
    _check_both_footprints(sm, fn, lambda i, o, c: lib.dc_stockham(fn, i, o, n, BLOCKS, c, None), x, _want(fn, n, x),
                           f"Stockham {ST_FNS[fn]} N={n} build={build!r}")


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("fn", [3, 4])
@pytest.mark.parametrize("n", R2C_L)
def test_r2c_c2r_fill_call_drain(sm, n, fn, build):
    """<<<37, L/4>>> on L + 1 float2 (RC:349-365): do_FFT_Stockham_R2C_C2R<FFT_L, FFT_forward> on 2L reals is the packed half
    spectrum with element 0 = (DC, Nyquist) (S5); <FFT_L, FFT_inverse> on such a packed spectrum (here arbitrary) is (2L / 2) times
    the irfft (S6).  Drained right after the call."""
    lib = _lib(sm, build)
    x = _complex(np.random.default_rng(200 * n + fn), (BLOCKS, n))
    _check_both_footprints(sm, fn, lambda i, o, c: lib.dc_stockham(fn, i, o, n, BLOCKS, c, None), x, _want(fn, n, x),
                           f"{ST_FNS[fn]} L={n} build={build!r}")


# ------------------------------------------------------------------ registers forms
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("fn", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_stockham_registers(sm, n, fn, inverse, build):
    """do_FFT_Stockham_C2C_registers<FFT_N, D> (fn 0: results element t + m N/4) and _registers_out (fn 1: results where the last
    phase leaves them, at the element indices it returns), thread t holding inputs t + m N/4, N float2 of scratch as
    FFT_GPU_external passes it."""
    lib = _lib(sm, build)
    x = _complex(np.random.default_rng(300 * n + 10 * fn + inverse), (BLOCKS, n))
    _check_both_footprints(sm, 1, lambda i, o, c: lib.dc_stockham_registers(fn, inverse, i, o, n, BLOCKS, c, None), x,
                           ref.st_c2c(x, inverse=bool(inverse)), f"Stockham registers{'_out' if fn else ''} N={n} inverse={inverse} build={build!r}")


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("inv,reo", [(0, 1), (1, 1), (0, 0), (1, 0)])
@pytest.mark.parametrize("n", [256, 512, 1024, 2048, 4096])
def test_ct_dit_registers(sm, n, inv, reo, build):
    """do_SMFFT_CT_DIT_registers<P> for all 20 CT classes of N >= 256: inputs as INTEGRATION.md's snippet loads them (natural order:
    element t + m N/4; no reorder: element 4 t + m), results element t + m N/4, P::fft_sm_required float2 of scratch.  At N = 2048 /
    4096 this is not the path of _registers_out (OUT_PHASED = false)."""
    lib = _lib(sm, build)
    x = _complex(np.random.default_rng(400 * n + 10 * inv + reo), (BLOCKS, n))
    _check_both_footprints(sm, 1, lambda i, o, c: lib.dc_ct_registers(inv, reo, i, o, n, BLOCKS, c, None), x,
                           ref.ct_c2c(x, bool(inv), bool(reo)), f"CT registers N={n} inv={inv} reorder={reo} build={build!r}")


# ------------------------------------------------------------------ the two-argument kernel at the lengths upstream lacks
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("n", [32, 64, 128])
def test_fft_gpu_external_small(sm, n, build):
    """FFT_GPU_external<FFT_N><<<37, N/4, N*8>>>(in, out) for N = 32, 64, 128 (SM_FFT_stockham_parameters.hpp admits them): blocks
    of 8, 16 and 32 threads holding one transform each."""
    lib = _lib(sm, build)
    x = _complex(np.random.default_rng(500 + n), (BLOCKS, n))
    got, _ = _launch(sm, lambda i, o, c: lib.dc_fft_gpu_external(i, o, n, BLOCKS, None), x, np.complex64, x.shape)
    ref.assert_close_fp32(got, ref.st_c2c(x, inverse=True), f"FFT_GPU_external N={n} build={build!r}")


# ------------------------------------------------------------------ chains with a runtime count
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("fn,n", [(1, n) for n in SIZES] + [(3, n) for n in R2C_L])
def test_chain_in_a_runtime_loop(sm, n, fn, build):
    """fn 1: do_FFT_Stockham_C2C forward then inverse, k times (N^k x); fn 3: do_FFT_Stockham_R2C_C2R forward then inverse on the
    same LDS array, k times (L^k x, S6) -- k a kernel argument, so twiddles hoisted out of the loop and the wave's scalar state carried
    across it are exercised.  2k applications: tolerance times sqrt(2k)."""
    lib = _lib(sm, build)
    x = _complex(np.random.default_rng(600 * n + fn), (BLOCKS, n))
    for rounds in (1, 3):
        got, _ = _launch(sm, lambda i, o, c: lib.dc_chain(fn, i, o, n, BLOCKS, rounds, None), x, np.complex64, x.shape)
        l2, mx = ref.fft_errors(got / np.float32(n) ** rounds, x.astype(np.complex128))
        k = 2 * rounds
        assert l2 <= ref.REL_L2_TOL * k ** 0.5 and mx <= ref.MAX_ABS_TOL * k ** 0.5, (n, fn, rounds, l2, mx)


# ------------------------------------------------------------------ the tiled contract
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("fn,n", [(fn, n) for fn in (0, 1, 2) for n in SIZES] + [(fn, n) for fn in (3, 4) for n in R2C_L])
def test_tiled_stockham_and_r2c(sm, n, fn, build):
    """smfft::tiled::do_FFT_Stockham_mk6 / _C2C / _R2C_C2R: 256 threads, 4096 / N transforms per workgroup, transform j at
    s[j * 17N/16 + n] (smfft::Geometry<N>::SF -- the Stockham classes have no fft_region) of 4352 float2."""
    lib = _lib(sm, build)
    nffts = BLOCKS * (4096 // n)
    x = _complex(np.random.default_rng(700 * n + fn), (nffts, n))
    _check_both_footprints(sm, fn, lambda i, o, c: lib.dc_tiled(fn, i, o, n, nffts, c, None), x, _want(fn, n, x),
                           f"tiled {ST_FNS[fn]} N={n} build={build!r}")


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("inv,reo", [(0, 1), (1, 1), (0, 0), (1, 0)])
@pytest.mark.parametrize("n", SIZES)
def test_tiled_ct_dit(sm, n, inv, reo, build):
    """smfft::tiled::do_SMFFT_CT_DIT<FFT_<N>_{forward,inverse}{,_noreorder}>, all 32 classes: the tiled layout of
    test_tiled_stockham_and_r2c (256 threads, 4096 / N transforms per workgroup at a stride of 17N/16, 4352 float2), the transform of
    the class's direction and order (S1 / S2)."""
    lib = _lib(sm, build)
    nffts = BLOCKS * (4096 // n)
    x = _complex(np.random.default_rng(750 * n + 10 * inv + reo), (nffts, n))
    _check_both_footprints(sm, 1, lambda i, o, c: lib.dc_tiled_ct(inv, reo, i, o, n, nffts, c, None), x,
                           ref.ct_c2c(x, bool(inv), bool(reo)), f"tiled CT N={n} inv={inv} reorder={reo} build={build!r}")


# ------------------------------------------------------------------ full occupancy
FULL = [("stockham", 0, 1024), ("stockham", 1, 512), ("stockham", 1, 2048), ("stockham", 2, 4096), ("stockham", 3, 1024),
        ("stockham", 4, 2048), ("registers", 0, 2048), ("registers", 1, 4096), ("ct_registers", 0, 2048),
        ("ct_registers", 1, 4096), ("tiled", 1, 1024), ("tiled", 3, 512)]


@pytest.mark.parametrize("family,fn,n", FULL)
def test_full_occupancy(sm, family, fn, n):
    """About 2^22 elements -- every CU full of blocks, several rounds: each family against fp64, and a second launch gives the same
    bits.  The C2C cases of N >= 512 (several waves per block) drain right after the call: a missing trailing barrier races here."""
    lib = _lib(sm)
    nffts = (1 << 22) // n + (BLOCKS if family != "tiled" else 0)
    x = _complex(np.random.default_rng(800 * n + fn), (nffts, n))
    if family == "stockham":
        call, want = (lambda i, o, c: lib.dc_stockham(fn, i, o, n, nffts, None, None)), _want(fn, n, x)
    elif family == "registers":
        call, want = (lambda i, o, c: lib.dc_stockham_registers(fn, 0, i, o, n, nffts, None, None)), ref.st_c2c(x, inverse=False)
    elif family == "ct_registers":
        call, want = (lambda i, o, c: lib.dc_ct_registers(0, fn, i, o, n, nffts, None, None)), ref.ct_c2c(x, False, bool(fn))
    else:
        call, want = (lambda i, o, c: lib.dc_tiled(fn, i, o, n, nffts, None, None)), _want(fn, n, x)
    first, _ = _launch(sm, call, x, np.complex64, x.shape)
    _check(fn if family in ("stockham", "tiled") else 1, first, want, f"{family} fn={fn} N={n}")
    second, _ = _launch(sm, call, x, np.complex64, x.shape)
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32)), f"{family} fn={fn} N={n}: second launch differs"


# ------------------------------------------------------------------ the header's `multiple` kernels, NREUSES = 3
def _nreuses3(sm):
    lib = _lib(sm, "_nreuses3")
    assert lib.dc_nreuses() == 3
    return lib


@pytest.mark.parametrize("inv,reo", [(0, 1), (1, 1), (0, 0), (1, 0)])
@pytest.mark.parametrize("n,wave64", [(n, 0) for n in SIZES] + [(n, 1) for n in (32, 64, 128)])
def test_ct_multiple_three_applications(sm, n, wave64, inv, reo):
    """SMFFT_DIT_multiple<P> built with NREUSES = 3, every CT class including the _wave64 ones, in the reference's launch shape:
    three applications of the fp64 transform."""
    lib = _nreuses3(sm)
    per = max(1, (256 if wave64 else 128) // n)
    nffts = BLOCKS * per
    x = _complex(np.random.default_rng(900 * n + 10 * inv + reo + 5 * wave64), (nffts, n))
    got, _ = _launch(sm, lambda i, o, c: lib.dc_ct_multiple(inv, reo, wave64, i, o, n, nffts, None), x, np.complex64, x.shape)
    want = x
    for _ in range(3):
        want = ref.ct_c2c(want, bool(inv), bool(reo))
    l2, mx = ref.fft_errors(got, want)
    assert l2 <= ref.REL_L2_TOL * 3 ** 0.5 and mx <= ref.MAX_ABS_TOL * 3 ** 0.5, (n, wave64, inv, reo, l2, mx)


@pytest.mark.parametrize("n", SIZES)
def test_fft_gpu_multiple_three_applications(sm, n):
    """FFT_GPU_multiple<FFT_N><<<37, N/4, N*8>>> built with NREUSES = 3: three applications of the + sign transform (S3)."""
    lib = _nreuses3(sm)
    x = _complex(np.random.default_rng(1000 + n), (BLOCKS, n))
    got, _ = _launch(sm, lambda i, o, c: lib.dc_fft_gpu_multiple(i, o, n, BLOCKS, None), x, np.complex64, x.shape)
    want = ref.st_c2c(ref.st_c2c(ref.st_c2c(x, True), True), True)
    l2, mx = ref.fft_errors(got, want)
    assert l2 <= ref.REL_L2_TOL * 3 ** 0.5 and mx <= ref.MAX_ABS_TOL * 3 ** 0.5, (n, l2, mx)


@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("n", R2C_L)
def test_rc_multiple_three_applications(sm, n, inverse):
    """FFT_GPU_R2C_C2R_multiple<FFT_L, D><<<37, L/4>>> built with NREUSES = 3: the output of one application, read as 2L reals
    (forward) or as L packed complex (inverse), is the next one's input, as test_r2c_multiple_k_applications feeds it."""
    lib = _nreuses3(sm)
    x = _complex(np.random.default_rng(1100 + 2 * n + inverse), (BLOCKS, n))
    got, _ = _launch(sm, lambda i, o, c: lib.dc_rc_multiple(inverse, i, o, n, BLOCKS, None), x, np.complex64, x.shape)
    want = x.astype(np.complex128)
    for _ in range(3):
        if inverse:
            want = ref.c2r_packed(want).view(np.complex128).reshape(BLOCKS, n)
        else:
            want = ref.r2c_packed(want.view(np.float64).reshape(BLOCKS, 2 * n))
    l2, mx = ref.fft_errors(got, want)
    assert l2 <= ref.REL_L2_TOL * 3 ** 0.5 and mx <= ref.MAX_ABS_TOL * 3 ** 0.5, (n, inverse, l2, mx)

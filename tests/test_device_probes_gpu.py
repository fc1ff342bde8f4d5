"""Every function of the header-only device API (include/smfft_device.hpp; tests/device_function_inventory.py) per output element, on
zero-mean data, and in isolation from the rest of its batch: the checks A1, A2, A3 and B of tests/test_probes_gpu.py, with its
definitions, ceilings and helpers, over the cases of tests/probe_cases.py HEADER_CASES.

The cases drive the entry points that already take a batch and a stream: the dc_* launchers of tests/hip/device_contract.hip in its four
header builds (and the NREUSES = 3 build for the `multiple` kernels), the smfft_example_* entries of examples/ in theirs (the
_wave64small build among them) and smfft_example_dif_ct.  The default build runs every case; a switch build runs only the classes whose
code its switch changes (probe_cases.switch_changes states the rule).

A1  The identity batch (R2C: real impulses; C2R: the packed unit spectra), per element against k * 3 * (log2 N + 2) * 2^-24 of the
    row's largest |ref|.  For a C2C transform applied once the expected output of impulse j is a pure twiddle, read from one fp64
    table at the integer product (natural order j m, no reorder rev(j) m, DIF j rev(m)): no fp64 transform of the identity is built.
A2  One fixed-seed Gaussian batch of >= 2^21 values: relL2 <= 5e-7 sqrt(k).
A3  tests/accuracy_ratchet.json holds the figures of every case (tools/accuracy_ratchet.py --header measures them); 1.25 x is the limit.
B   A Gaussian batch of 37 blocks of the entry's launch shape, every row scaled by 2^e (adjacent rows differ in e), some rows poisoned
    with NaN / +-Inf: row 0, the last row of block 0 and the first of block 1, a row inside a block that holds several transforms
    (N <= 128, _wave64, tiled), a mid-batch row with clean neighbours and the last transform.  Clean rows must be exactly 2^e times
    their unscaled output, poisoned rows entirely non-finite."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import probe_cases as pc
from tests import test_probes_gpu as tp

pytestmark = pytest.mark.gpu

ISO_BLOCKS = 37
_VP, _I = ctypes.c_void_p, ctypes.c_int
_ARGTYPES = {
    "dc_stockham": [_I, _VP, _VP, _I, _I, _VP, _VP],
    "dc_tiled": [_I, _VP, _VP, _I, _I, _VP, _VP],
    "dc_tiled_ct": [_I, _I, _VP, _VP, _I, _I, _VP, _VP],
    "dc_stockham_registers": [_I, _I, _VP, _VP, _I, _I, _VP, _VP],
    "dc_ct_registers": [_I, _I, _VP, _VP, _I, _I, _VP, _VP],
    "dc_fft_gpu_external": [_VP, _VP, _I, _I, _VP],
    "dc_ct_multiple": [_I, _I, _I, _VP, _VP, _I, _I, _VP],
    "dc_fft_gpu_multiple": [_VP, _VP, _I, _I, _VP],
    "dc_rc_multiple": [_I, _VP, _VP, _I, _I, _VP],
    "dc_nreuses": [],
    "smfft_example_reference_shape_ct": [_VP, _VP, _I, _I, _I, _I, _I, _VP],
    "smfft_example_reference_shape_ct_times": [_VP, _VP, _I, _I, _I, _I, _I, _VP],
    "smfft_example_reference_shape_st": [_VP, _VP, _I, _I, _VP],
    "smfft_example_reference_shape_rc": [_VP, _VP, _I, _I, _I, _VP],
    "smfft_example_dif_ct": [_VP, _VP, _I, _I, _I, _I, _VP],
}


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    assert smfft_amd.lib.smfft_device_count() >= 1, "no HIP device"
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def ratchet():
    with open(tp.RATCHET) as f:
        return json.load(f)


_LIBS = {}


def _lib(sm, stem, build):
    name = f"{stem}{'' if build == 'default' else '_' + build}.so"
    if name not in _LIBS:
        path = os.path.join(os.path.dirname(sm.LIB_PATH), name)
        if not os.path.exists(path):
            pytest.fail(f"{name} is missing: it is built by smfft_amd/csrc/Makefile -- a GPU run without it is a broken build, not a skip")
        lib = ctypes.CDLL(path)
        for fn, args in _ARGTYPES.items():
            if hasattr(lib, fn):
                getattr(lib, fn).argtypes = args
        _LIBS[name] = lib
    return _LIBS[name]


def _call(sm, case, din, dout, rows):
    """launch the case's entry point on `rows` transforms -> status"""
    f, n, inv, reo = case.func, case.n, case.inv, case.reo
    dc = lambda: _lib(sm, "libsmfft_device_contract", case.build)      # noqa: E731
    ex = lambda: _lib(sm, "libsmfft_examples", case.build)             # noqa: E731
    if f in ("ct", "ct_ext", "ct_wave64", "ct_ext_wave64"):
        which = {"ct": 0, "ct_ext": 1, "ct_wave64": 2, "ct_ext_wave64": 3}[f]
        return ex().smfft_example_reference_shape_ct(din, dout, n, rows, inv, reo, which, None)
    if f == "ct_times":
        return ex().smfft_example_reference_shape_ct_times(din, dout, n, rows, reo, case.k, 0, None)
    if f == "ct_registers":
        return dc().dc_ct_registers(inv, reo, din, dout, n, rows, None, None)
    if f in ("ct_multiple", "ct_multiple_wave64", "st_multiple", "rc_multiple"):
        lib = _lib(sm, "libsmfft_device_contract", "nreuses3")
        assert lib.dc_nreuses() == case.k == 3
        if f == "st_multiple":
            return lib.dc_fft_gpu_multiple(din, dout, n, rows, None)
        if f == "rc_multiple":
            return lib.dc_rc_multiple(inv, din, dout, n, rows, None)
        return lib.dc_ct_multiple(inv, reo, int(case.wave64), din, dout, n, rows, None)
    if f in ("st_mk6", "st_c2c", "rc"):
        return dc().dc_stockham({"st_mk6": 0, "st_c2c": 1 + inv, "rc": 3 + inv}[f], din, dout, n, rows, None, None)
    if f in ("st_registers", "st_registers_out"):
        return dc().dc_stockham_registers(int(f == "st_registers_out"), inv, din, dout, n, rows, None, None)
    if f == "st_ext":
        if n <= 128:
            return dc().dc_fft_gpu_external(din, dout, n, rows, None)
        return ex().smfft_example_reference_shape_st(din, dout, n, rows, None)
    if f == "rc_ext":
        return ex().smfft_example_reference_shape_rc(din, dout, 2 * n, rows, inv, None)
    if f == "tiled_ct":
        return dc().dc_tiled_ct(inv, reo, din, dout, n, rows, None, None)
    if f in ("tiled_mk6", "tiled_c2c", "tiled_rc"):
        return dc().dc_tiled({"tiled_mk6": 0, "tiled_c2c": 1 + inv, "tiled_rc": 3 + inv}[f], din, dout, n, rows, None, None)
    if f in ("dif", "dif_registers", "dif_wave64"):
        return ex().smfft_example_dif_ct(din, dout, n, rows, inv, {"dif": 0, "dif_registers": 1, "dif_wave64": 2}[f], None)
    raise AssertionError(case)


def _transform(sm, case, x):
    """the case's entry point on the rows of x (complex64; float32 reals for R2C), padded with zero rows to whole blocks -> its output
    rows (complex64; float32 reals for C2R), every output word prefilled with NaN"""
    rows = x.shape[0]
    per = case.per_block
    padded = -(-rows // per) * per
    xs = np.zeros((padded,) + x.shape[1:], x.dtype)
    xs[:rows] = x
    din, dout = sm.DeviceBuffer.from_host(xs), sm.DeviceBuffer(xs.nbytes)
    try:
        assert sm.lib.smfft_memset(dout.ptr, 0xFF, dout.nbytes) == 0
        assert _call(sm, case, din.ptr, dout.ptr, padded) == 0, case.id
        assert sm.lib.smfft_synchronize() == 0
        if case.rc and case.inv:
            return dout.to_host(np.float32, (padded, 2 * case.n))[:rows]
        return dout.to_host(np.complex64, (padded, case.n))[:rows]
    finally:
        din.free()
        dout.free()


def _twiddle_probe_errors(sm, case):
    """A1 of a C2C case applied once: the identity, and the expected output of impulse j at m, W_N^{-+ (a(j) b(m) mod N)}, from one
    fp64 table at the integer product (a, b: the identity or the bit reversal of the case's order).  Every |ref| is 1."""
    n = case.n
    table = np.exp((1 if case.inv else -1) * 2j * np.pi * np.arange(n) / n)
    rev = tp.ref.bitrev_indices(n).astype(np.int64)
    idx = np.arange(n, dtype=np.int64)
    a = rev if (not case.reo and not case.func.startswith("dif")) else idx
    b = rev if case.func.startswith("dif") else idx
    got = _transform(sm, case, np.eye(n, dtype=np.complex64))
    worst, sq = 0.0, 0.0
    step = max(1, (1 << 22) // n)
    for j0 in range(0, n, step):
        j = slice(j0, min(n, j0 + step))
        err = np.abs(got[j] - table[(a[j, None] * b[None, :]) & (n - 1)]).ravel()
        worst = max(worst, float(err.max()))
        sq += float(np.dot(err, err))
    return worst, float(np.sqrt(sq / (n * n)))


def probe_errors(sm, case):
    """(largest, rms) of the per-element errors |err| / max |ref_row| of the DFT-matrix probe"""
    if not case.rc and case.k == 1:
        return _twiddle_probe_errors(sm, case)
    lc = case.as_lib()
    x = tp.probe_batch(lc)
    got = _transform(sm, case, x.view(np.complex64) if lc.real_in else x)
    want = tp._reference(lc, x)
    assert got.shape == want.shape, (got.shape, want.shape)
    rel = np.abs(got.astype(want.dtype) - want) / np.abs(want).max(axis=1)[:, None]
    return float(rel.max()), float(np.sqrt(np.mean(rel ** 2)))


def gauss_error(sm, case):
    lc = case.as_lib()
    x = tp.gauss_batch(lc)
    got = _transform(sm, case, x.view(np.complex64) if lc.real_in else x)
    want = tp._reference(lc, x)
    return float(np.linalg.norm(got.astype(want.dtype) - want) / np.linalg.norm(want))


# ---------------------------------------------------------------------------------------------------- A1 / A2 / A3
@pytest.mark.parametrize("case", pc.HEADER_CASES, ids=lambda c: c.id)
def test_dft_matrix_probe(sm, ratchet, case):
    per_elem, rms = probe_errors(sm, case)
    ceiling = pc.probe_ceiling(case.length, case.k)
    assert per_elem <= ceiling, f"{case.id}: per-element error {per_elem:.3e} above the twiddle-chain ceiling {ceiling:.3e}"
    tp._ratchet_check(ratchet, case, "probe_max", per_elem)
    tp._ratchet_check(ratchet, case, "probe_rms", rms)


@pytest.mark.parametrize("case", pc.HEADER_CASES, ids=lambda c: c.id)
def test_zero_mean_accuracy(sm, ratchet, case):
    l2 = gauss_error(sm, case)
    assert l2 <= pc.gauss_bound(case.k), f"{case.id}: Gaussian relL2 {l2:.3e} above {pc.gauss_bound(case.k):.3e}"
    tp._ratchet_check(ratchet, case, "gauss_rel_l2", l2)


# ---------------------------------------------------------------------------------------------------- B: isolation, exact scaling
def iso_rows(case):
    """(rows of the batch, the rows to poison): 37 blocks of the entry's launch shape"""
    per = case.per_block
    rows = ISO_BLOCKS * per
    poison = {0, per - 1, per, 17 * per + per // 2, rows - 1}
    if per > 2:
        poison.add(2 * per + per // 2)             # inside a block of several transforms, its neighbours clean
    return rows, sorted(poison)


@pytest.mark.parametrize("case", [c for c in pc.HEADER_CASES], ids=lambda c: c.id[:-3])
def test_isolation_and_exact_scaling(sm, case):
    rows, poison = iso_rows(case)
    lc = case.as_lib()
    w = tp._width_in(lc)
    rng = np.random.default_rng([rows, case.n, case.inv, case.reo, len(case.func), len(case.build)])
    if lc.real_in:
        x = rng.standard_normal((rows, w)).astype(np.float32)
    else:
        x = (rng.standard_normal((rows, w)) + 1j * rng.standard_normal((rows, w))).astype(np.complex64)
    e = np.array([tp.SCALES[r % len(tp.SCALES)] for r in range(rows)])
    y, kinds = tp.poisoned_batch(x, e, poison, lc.real_in)
    view = (lambda a: a.view(np.complex64)) if lc.real_in else (lambda a: a)
    clean = _transform(sm, case, view(x))
    dirty = _transform(sm, case, view(y))
    tp.assert_isolated_and_exact(clean, dirty, e, kinds, lc.real_in, lc.real_out, case.id[:-3])

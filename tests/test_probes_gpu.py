"""Every transform kernel per output element, on zero-mean data, and in isolation from the rest of its batch.

A1  DFT-matrix probes (test_dft_matrix_probe).  The batch is the N x N identity (R2C: real impulses; C2R: the N packed unit spectra
    -- DC, Nyquist, then a real and an imaginary unit at every bin 1 ... N/2 - 1), so the output is the DFT matrix and every path
    from an input to an output carries the same weight: an error in one twiddle of one butterfly cannot average away.  The expected
    output is oracle/np_reference.py's statement in fp64 of the same batch (bit reversal of the no-reorder and DIF kernels
    included).  Ceiling per element, relative to the largest |ref| of its row:
        |err| <= k * 3 * (log2 N + 2) * 2^-24 * max |ref_row|
    Derivation, for a unit impulse (every value of every stage is a single nonzero path, of magnitude max |ref_row| = 1 at k = 1):
    a radix-2 stage computes a + w b.  The table's twiddle w is within 0.5 ulp of exp(-2 pi i m / 4096) (tests/test_twiddle_table.py),
    an error <= 0.5 * 2^-24 relative; the complex product w b rounds with relative error <= sqrt(2) 2^-24 < 1.5 * 2^-24; the sum
    adds <= 2^-24 relative.  So a stage adds at most 3 * 2^-24 of max |ref_row|, log2 N stages add 3 log2 N 2^-24, and the Hermitian
    step of R2C / C2R (one table twiddle and one complex product; its 1/2 scalings are exact) adds at most two stages' worth.  A
    second application maps the first one's error through a DFT, whose gain on the largest element is the same N as its gain on
    max |ref_row|: k applications add k ceilings.  Higher radices fold the same roundings into fewer operations, so the radix-2
    chain bounds them.
    The `large` kind (N = 8192, 16384) runs the identity in chunks of 2^23 elements (the whole of it would take ~12 GiB of host
    memory at 16384) and takes the expected output of impulse j, exactly W_N^{-+(j m mod N)} at output m, from one fp64 table
    indexed by the integer product: the same ceiling and rms, every |ref| = 1.
A2  Zero-mean accuracy (test_zero_mean_accuracy): one fixed-seed complex (R2C: real) Gaussian batch of >= 2^21 values, aggregate
    relL2 ||Y - Y64||_F / ||Y64||_F <= 5e-7 sqrt(k), the library's per-FFT bound.
A3  Ratchet: tests/accuracy_ratchet.json holds, per case id, the figures A1 and A2 measured on an MI355X (tools/accuracy_ratchet.py
    writes it).  The kernels are deterministic, so only a change of a kernel or of the compiler moves them; a figure above 1.25 x its
    entry fails, and so does a case without an entry.
B   Isolation and exact scaling (test_isolation_and_exact_scaling): a clean Gaussian batch, then the same batch with some rows
    poisoned (a complex NaN, a +Inf, a -Inf imaginary part at one position) and every other row scaled by 2^e, e in {-40, -13, 0, 11,
    40}.  Every unpoisoned output row must be ldexp(clean row, e) to the bit -- rows do not interact and the transform is exactly
    homogeneous -- and every element of a poisoned row must have a non-finite component (both, for a complex NaN).  The poisoned rows
    are row 0, a row inside the first workgroup's tile, the first and the last row of the ragged last tile, the last transform and, on
    the `multiple` paths, the rows on both sides of every chain the balanced schedule cuts.  The `multiple` paths run k = 1, 2, 3 under
    the plain schedule and under smfft_set_multiple_balance(2) and (7).
    The `large` kernels are persistent: G = smfft_amd.large.grid(N) workgroups, workgroup w transforms rows w, w + G, w + 2G, ...
    in turn and carries its registers and LDS image from one to the next.  Their batch is 3G + G/2 rows (3 or 4 rounds, the last
    one ragged), poisoned in every round -- row 0, row G - 1, the first and the last row of the ragged round among them -- with row
    f + G clean after several poisoned rows f, so that what a workgroup carries into its next FFT reaches a finite row.  Their
    exponents differ between rows f and f + 1 and between rows f and f + G, so a leak between them cannot scale exactly.
    FIR filter banks (test_fir_*): every channel scaled by 2^e scales its outputs exactly; a complex NaN at one sample turns exactly
    the stored windows of the segments that load it (tools/fir_plan_model.py) into NaN for every filter and leaves every other
    word alone; a NaN tap makes exactly its filter's spectrum row and output rows NaN."""
import json
import os
import sys

import numpy as np
import pytest

from oracle import np_reference as ref
from tests import probe_cases as pc
from tests.fir_gpu_harness import GRID_CAP

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fir_plan_model as fm  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATCHET = os.path.join(ROOT, "tests", "accuracy_ratchet.json")
NREUSES = 100                  # the `multiple` paths transform the first nFFTs / 100 slots
SCALES = (-40, -13, 0, 11, 40)
LARGE_SCALES = (-40, 11, -13, 40)   # the `large` kind's, chosen by the parities of the row and of its round
BALANCES = (0, 2, 7)           # 0: one chain per workgroup; g >= 2: a persistent grid of g workgroups


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    assert smfft_amd.lib.smfft_device_count() >= 1, "no HIP device"
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def ratchet():
    with open(RATCHET) as f:
        return json.load(f)


# ---------------------------------------------------------------------------------------------------- running a case
def _width_in(case):
    return case.n // 2 if case.real_out else case.n


def _slot_unit(case):
    """the CT `multiple` launches round their slots down to pairs (N = 64) / quads (N = 32): smfft_api.hip, ct_multiple_slots"""
    if case.kind.startswith("ct_multiple"):
        return 4 if case.n == 32 else 2 if case.n == 64 else 1
    return 1


def _multiple(sm, case, x, k, balance):
    """smfft_launch on the first rows = len(x) slots of a batch of nFFTs = 100 rows + 37 (only those are transformed): device
    buffers of the whole batch, the slots copied in and out"""
    rows = x.shape[0]
    assert rows % _slot_unit(case) == 0
    nffts = NREUSES * rows + 37
    row_bytes = case.n * 4 if case.real_in else (case.n // 2 if case.real_out else case.n) * 8
    family, path = {"ct": ("ct", "multiple"), "st": ("st", "multiple"), "r2c": ("rc", "multiple"), "c2r": ("rc", "multiple")}[case.kind.split("_")[0]]
    if case.kind == "ct_multiple_unfused":
        path = "multiple_unfused"
    out_dtype = np.float32 if case.real_out else np.complex64
    out_width = case.n if case.real_out else case.n // 2 if case.real_in else case.n
    din, dout = sm.DeviceBuffer(nffts * row_bytes), sm.DeviceBuffer(nffts * row_bytes)
    try:
        assert sm.lib.smfft_memset(din.ptr, 0, din.nbytes) == 0
        assert sm.lib.smfft_memset(dout.ptr, 0xFF, dout.nbytes) == 0
        xs = np.ascontiguousarray(x)
        assert sm.lib.smfft_memcpy_h2d(din.ptr, xs.ctypes.data, xs.nbytes) == 0
        sm.lib.smfft_set_nreuses(k)
        sm.lib.smfft_set_multiple_balance(balance)
        sm.launch(family, path, din.ptr, dout.ptr, case.n, nffts, inverse=bool(case.inv), reorder=bool(case.reo))
        assert sm.lib.smfft_synchronize() == 0
        return dout.to_host(out_dtype, (rows, out_width))
    finally:
        sm.lib.smfft_set_nreuses(0)
        sm.lib.smfft_set_multiple_balance(-1)
        din.free()
        dout.free()


def _transform(sm, case, x, k=None, balance=0):
    """the case's kernel on the rows of x (complex64; float32 for R2C) -> its output rows"""
    k = case.k if k is None else k
    if case.multiple:
        return _multiple(sm, case, x, k, balance)
    assert k == 1
    if case.kind == "ct_external":
        return sm.c2c(x, bool(case.inv), bool(case.reo))
    if case.kind == "st_external":
        return sm.stockham_c2c(x, inverse=bool(case.inv))
    if case.kind == "dif":
        return sm.c2c_dif(x, inverse=bool(case.inv))
    if case.kind == "r2c_external":
        return sm.r2c(x)
    if case.kind == "c2r_external":
        return sm.c2r(x)
    if case.kind == "large":
        from smfft_amd import large
        return large.c2c(x, bool(case.inv))
    raise AssertionError(case)


def _reference(case, x):
    """k applications of the case's transform in fp64 (oracle/np_reference.py)"""
    y = np.asarray(x, np.float64 if case.real_in else np.complex128)
    rows = y.shape[0]
    for _ in range(case.k):
        if case.real_in:
            y = ref.r2c_packed(y)
            last = y
            y = y.view(np.float64).reshape(rows, case.n)
        elif case.real_out:
            y = ref.c2r_packed(y)
            last = y
            y = y.view(np.complex128).reshape(rows, case.n // 2)
        elif case.kind == "dif":
            y = ref.ct_c2c(y, bool(case.inv), True)[:, ref.bitrev_indices(case.n)]
            last = y
        else:
            y = ref.ct_c2c(y, bool(case.inv), bool(case.reo))
            last = y
    return last


def probe_batch(case):
    """A1's input: the identity (real impulses for R2C), or for C2R the N packed unit spectra"""
    n = case.n
    if case.real_in:
        return np.eye(n, dtype=np.float32)
    if case.real_out:
        h = n // 2
        x = np.zeros((n, h), np.complex64)
        x[0, 0] = 1                                  # DC
        x[1, 0] = 1j                                 # Nyquist: the imaginary part of element 0
        m = np.arange(1, h)
        x[1 + m, m] = 1                              # a real unit at bin m
        x[h + m, m] = 1j                             # an imaginary unit at bin m
        return x
    return np.eye(n, dtype=np.complex64)


def gauss_batch(case):
    """A2's input: >= 2^21 values, fixed seed per case"""
    rng = np.random.default_rng([ord(c) for c in case.id])
    if case.real_in:
        return rng.standard_normal((2 ** 22 // case.n, case.n)).astype(np.float32)
    w = _width_in(case)
    return (rng.standard_normal((2 ** 21 // w, w)) + 1j * rng.standard_normal((2 ** 21 // w, w))).astype(np.complex64)


LARGE_PROBE_CHUNK = 1 << 23    # elements of the identity per call of the `large` kind's probe


def _large_probe_errors(sm, case):
    """A1 of the `large` kind: the N x N identity in chunks of impulses.  Output m of impulse j is W_N^{-+(j m mod N)}, read from one
    fp64 table at the integer product; every |ref| is 1 (to fp64 rounding), so max |ref_row| = 1 and |err| is the relative error."""
    n = case.n
    table = np.exp((1 if case.inv else -1) * 2j * np.pi * np.arange(n) / n)
    m = np.arange(n, dtype=np.int64)
    worst, sq = 0.0, 0.0
    step = max(1, LARGE_PROBE_CHUNK // n)
    for j0 in range(0, n, step):
        j = np.arange(j0, min(n, j0 + step), dtype=np.int64)
        x = np.zeros((len(j), n), np.complex64)
        x[np.arange(len(j)), j] = 1
        got = _transform(sm, case, x)
        err = np.abs(got - table[(j[:, None] * m) & (n - 1)]).ravel()
        worst = max(worst, float(err.max()))
        sq += float(np.dot(err, err))
    return worst, float(np.sqrt(sq / (n * n)))


def probe_errors(sm, case):
    """(largest, rms) of the per-element errors |err| / max |ref_row| of the DFT-matrix probe (at k = 1 the rms is the batch's relL2:
    every |ref| is 1 there)"""
    if case.kind == "large":
        return _large_probe_errors(sm, case)
    x = probe_batch(case)
    got = _transform(sm, case, x)
    want = _reference(case, x)
    assert got.shape == want.shape
    err = np.abs(got.astype(want.dtype) - want)
    rowmax = np.abs(want).max(axis=1)
    assert (rowmax > 0).all()
    rel = err / rowmax[:, None]
    return float(rel.max()), float(np.sqrt(np.mean(rel ** 2)))


def gauss_error(sm, case):
    x = gauss_batch(case)
    got = _transform(sm, case, x)
    want = _reference(case, x)
    return float(np.linalg.norm(got.astype(want.dtype) - want) / np.linalg.norm(want))


def _ratchet_check(ratchet, case, key, value):
    assert case.id in ratchet, f"{case.id}: no entry in tests/accuracy_ratchet.json (tools/accuracy_ratchet.py measures it)"
    limit = pc.RATCHET_SLACK * ratchet[case.id][key]
    assert value <= limit, f"{case.id}: {key} = {value:.3e} above {pc.RATCHET_SLACK} x the committed {ratchet[case.id][key]:.3e}"


# ---------------------------------------------------------------------------------------------------- A1 / A2 / A3
@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.id)
def test_dft_matrix_probe(sm, ratchet, case):
    per_elem, rms = probe_errors(sm, case)
    ceiling = pc.probe_ceiling(case.n, case.k)
    assert per_elem <= ceiling, f"{case.id}: per-element error {per_elem:.3e} above the twiddle-chain ceiling {ceiling:.3e}"
    _ratchet_check(ratchet, case, "probe_max", per_elem)
    _ratchet_check(ratchet, case, "probe_rms", rms)


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.id)
def test_zero_mean_accuracy(sm, ratchet, case):
    l2 = gauss_error(sm, case)
    assert l2 <= pc.gauss_bound(case.k), f"{case.id}: Gaussian relL2 {l2:.3e} above {pc.gauss_bound(case.k):.3e}"
    _ratchet_check(ratchet, case, "gauss_rel_l2", l2)


# ---------------------------------------------------------------------------------------------------- B: isolation, exact scaling
def _cut_chains(ntiles, reuses, g):
    """chains a balanced launch over g workgroups cuts, with the application they are cut at (smfft_inst.hip, launch_compact)"""
    total = ntiles * reuses
    per_wg = -(-total // g)
    return [(b // reuses, b % reuses) for b in range(per_wg, total, per_wg) if b % reuses]


def _large_iso_rows(n):
    """(G, rows of the batch, the rows to poison) of the `large` kind: 3G + G/2 rows.  Poisoned in round 0: 0, G/3, G - 1; round 1:
    G + G/2 + 1, 2G - 2; round 2: 2G + 5, 2G + G/2 + 3 (its workgroup's last FFT); the ragged round 3: its first row 3G and the last
    row.  Rows f + G are clean after f = 0, G/3, G - 1, G + G/2 + 1 and 2G + 5."""
    from smfft_amd import large
    g = large.grid(n)
    assert g >= 16, g
    rows = 3 * g + g // 2
    carried = (0, g // 3, g - 1, g + g // 2 + 1, 2 * g + 5)
    poison = set(carried) | {2 * g - 2, 2 * g + g // 2 + 3, 3 * g, rows - 1}
    for f in carried:
        assert f + g < rows and f + g not in poison, (g, f)
    return g, rows, sorted(poison)


def _iso_rows(case):
    """(rows of the batch, the rows to poison): 23 tiles, the last one half full"""
    if case.kind == "large":
        return _large_iso_rows(case.n)[1:]
    nc = case.n // 2 if case.kind[:3] in ("r2c", "c2r") else case.n
    tile = max(1, 1024 // nc) if case.multiple else 4096 // nc      # Geometry<N>: kCompactFfts / kFftsPerBlock
    ntiles = 23
    rows = ntiles * tile - (tile // 2 if tile > 1 else 0)
    poison = {0, tile // 2, (ntiles - 1) * tile, rows - 1}
    if case.multiple:
        for k in (2, 3):
            for g in BALANCES[1:]:
                for t, _ in _cut_chains(ntiles, k, g):
                    poison |= {t * tile - 1, t * tile}
    return rows, sorted(poison)


def _iso_cases():
    seen, out = set(), []
    for c in pc.CASES:
        key = (c.kind, c.n, c.inv, c.reo)
        if key not in seen:
            seen.add(key)
            out.append(c._replace(k=1))
    return out


def _non_finite(a):
    return ~np.isfinite(a)


@pytest.mark.parametrize("case", _iso_cases(), ids=lambda c: c.id[:-3])
def test_isolation_and_exact_scaling(sm, case):
    rows, poison = _iso_rows(case)
    rng = np.random.default_rng([rows, case.n, case.inv, case.reo, len(case.kind)])
    w = _width_in(case)
    if case.real_in:
        x = rng.standard_normal((rows, w)).astype(np.float32)
    else:
        x = (rng.standard_normal((rows, w)) + 1j * rng.standard_normal((rows, w))).astype(np.complex64)
    e = np.array([SCALES[r % len(SCALES)] for r in range(rows)])
    if case.kind == "large":
        g = _large_iso_rows(case.n)[0]
        e = np.array([LARGE_SCALES[(r & 1) | ((r // g) & 1) << 1] for r in range(rows)])
        assert (e[1:] != e[:-1]).all() and (e[g:] != e[:-g]).all(), "rows f, f + 1 and f + G need different exponents"
    y, kinds = poisoned_batch(x, e, poison, case.real_in)
    runs = [(k, g) for k in (1, 2, 3) for g in BALANCES] if case.multiple else [(1, 0)]
    for k, g in runs:
        what = f"{case.id[:-3]} k={k} balance={g}"
        clean = _transform(sm, case, x, k, g)
        dirty = _transform(sm, case, y, k, g)
        assert_isolated_and_exact(clean, dirty, e, kinds, case.real_in, case.real_out, what)


def poisoned_batch(x, e, poison, real_in):
    """(y, kinds): row r of x scaled by 2^e[r], then a complex NaN, a +Inf real part or a -Inf imaginary part (kinds[r]) at one
    position of each row in `poison` (the ends of a row among them; row 0 has its poison at 0)"""
    rows, w = x.shape
    y = np.ldexp(x.view(np.float32).reshape(rows, -1), e[:, None]).view(x.dtype)
    assert np.array_equal(np.ldexp(y.view(np.float32).reshape(rows, -1), -e[:, None]), x.view(np.float32).reshape(rows, -1))
    kinds = {}
    for i, r in enumerate(poison):
        p = (0, w - 1, w // 2 + 1, (17 * r + 5) % w)[i % 4]
        kind = ("nan", "inf", "neginf_imag")[i % 3]
        kinds[r] = kind
        if real_in:
            y[r, p] = {"nan": np.nan, "inf": np.inf, "neginf_imag": -np.inf}[kind]
        else:
            y[r, p] = {"nan": complex(np.nan, np.nan), "inf": complex(np.inf, y[r, p].imag),
                       "neginf_imag": complex(y[r, p].real, -np.inf)}[kind]
    return y, kinds


def assert_isolated_and_exact(clean, dirty, e, kinds, real_in, real_out, what):
    """every unpoisoned row of `dirty` is ldexp(its `clean` row, e) to the bit; every element of a poisoned row has a non-finite
    component (both, for a complex NaN into a complex transform; C2R: every real)"""
    rows = clean.shape[0]
    clean_mask = np.ones(rows, bool)
    clean_mask[list(kinds)] = False
    cf = clean.view(np.float32).reshape(rows, -1)
    df = dirty.view(np.float32).reshape(rows, -1)
    assert np.isfinite(cf).all(), f"{what}: the clean batch gave non-finite outputs"
    want = np.ldexp(cf, e[:, None]).view(np.uint32)
    bad = np.nonzero((want[clean_mask] != df[clean_mask].view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, f"{what}: unpoisoned rows {np.nonzero(clean_mask)[0][bad][:8].tolist()} are not 2^e x their clean rows"
    for r, kind in kinds.items():
        if real_out:
            assert _non_finite(dirty[r]).all(), f"{what}: row {r} ({kind}) has finite outputs"
            continue
        nf_re, nf_im = _non_finite(dirty[r].real), _non_finite(dirty[r].imag)
        if kind == "nan" and not real_in:
            assert (nf_re & nf_im).all(), f"{what}: row {r} (complex NaN) has an output with a finite component"
        else:
            assert (nf_re | nf_im).all(), f"{what}: row {r} ({kind}) has a finite output"


# ---------------------------------------------------------------------------------------------------- B: the FIR filter banks
FIR_MODES = ("convolve", "correlate")


def _fir_shapes():
    """(N, C, L, K, M): the grid-stride shape of test_fir_gpu.py::test_grid_stride_loop_with_wrapped_prefetch at every N (about 2.5 x
    the grid cap of tiles), and the uneven filter-group shapes of test_uneven_filter_groups (groups of 3, 3 and 1 filters)"""
    out = []
    for N in (256, 512, 1024, 2048, 4096):
        S = 10240 * (4096 // N) + 1
        out.append((N, 3, 2 * S - 1, 3, N - 1))
    out += [(4096, 2, 2 * 700 - 1, 7, 4095), (256, 2, 2 * (699 * 16 + 5) - 1, 7, 255)]
    return out


FIR_SHAPES = _fir_shapes()


def _fir_run(sm, x, h, N, mode):
    """(spectra, output) of fir_prepare + fir_launch through the device-pointer API"""
    C, L = x.shape
    K, M = h.shape
    dx, dh, dspec, dout = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer.from_host(h), sm.DeviceBuffer(K * N * 8), sm.DeviceBuffer(C * K * L * 8)
    try:
        assert sm.lib.smfft_memset(dout.ptr, 0xFF, dout.nbytes) == 0
        sm.fir_prepare(dh.ptr, dspec.ptr, M, K, N, mode)
        sm.fir_launch(dx.ptr, L, C, dspec.ptr, K, M, N, dout.ptr, mode)
        assert sm.lib.smfft_synchronize() == 0
        return dspec.to_host(np.complex64, (K, N)), dout.to_host(np.complex64, (C, K, L))
    finally:
        for b in (dx, dh, dspec, dout):
            b.free()


def _fir_inputs(N, C, L, K, M, mode):
    rng = np.random.default_rng([N, C, L, K, M, mode == "correlate"])
    x = (rng.standard_normal((C, L)) + 1j * rng.standard_normal((C, L))).astype(np.complex64)
    h = (rng.standard_normal((K, M)) + 1j * rng.standard_normal((K, M))).astype(np.complex64)
    return x, h


def _shape_id(s):
    return "N{}-C{}-L{}-K{}".format(*s[:4])


@pytest.fixture(scope="module")
def fir_clean(sm):
    cache = {}

    def get(shape, mode):
        if (shape, mode) not in cache:
            N, C, L, K, M = shape
            x, h = _fir_inputs(*shape, mode)
            spec, y = _fir_run(sm, x, h, N, mode)
            assert np.isfinite(y.view(np.float32)).all()
            cache.clear()
            cache[(shape, mode)] = (x, h, spec, y)
        return cache[(shape, mode)]
    return get


@pytest.mark.parametrize("mode", FIR_MODES)
@pytest.mark.parametrize("shape", FIR_SHAPES, ids=_shape_id)
def test_fir_channels_scale_exactly(sm, fir_clean, shape, mode):
    N, C, L, K, M = shape
    x, h, spec, y = fir_clean(shape, mode)
    e = np.array([SCALES[(c + 1) % len(SCALES)] for c in range(C)])
    xs = np.ldexp(x.view(np.float32).reshape(C, -1), e[:, None]).view(np.complex64)
    _, ys = _fir_run(sm, xs, h, N, mode)
    want = np.ldexp(y.view(np.float32).reshape(C, -1), e[:, None]).view(np.uint32)
    assert np.array_equal(ys.view(np.float32).reshape(C, -1).view(np.uint32), want), f"{_shape_id(shape)} {mode}: channels do not scale exactly"


def _nan_samples(w, C, N):
    """(channel, sample): a segment's first loaded sample, a mid-segment sample, the last sample, and (past the grid cap) a sample of
    a segment that a workgroup reaches on its grid-stride loop"""
    S, F = w.segments(), 4096 // N
    s1 = min(S - 1, 2 + next((s for s in range(S) if w.load_start(s) > 0), 0))
    mid = max(0, w.load_start(S // 2)) + N // 2
    out = [(C - 1, max(0, w.load_start(s1))), (0, mid if mid < w.L - 1 else w.L // 2), (C // 2, w.L - 1)]
    tiles = -(-S * C // F)
    if tiles > GRID_CAP:
        g = GRID_CAP * F + 5                    # the batch's segment index: tile >= GRID_CAP
        c, s = divmod(g, S)
        out.append((c, max(0, w.load_start(s)) + 7))
    return out


@pytest.mark.parametrize("mode", FIR_MODES)
@pytest.mark.parametrize("shape", FIR_SHAPES, ids=_shape_id)
def test_fir_nan_sample_reaches_exactly_its_windows(sm, fir_clean, shape, mode):
    """the kernel loads x[a + e] from a clamped address and selects zero outside [0, L): a NaN at x[0] or x[L - 1], the samples the
    clamp substitutes, must not leak into a segment through the substituted positions (every segment that reaches past an end of
    the channel loads that end sample itself, so the windows below are the same set either way; what the test pins down is that no
    other segment, channel or filter sees the NaN)"""
    N, C, L, K, M = shape
    x, h, spec, y = fir_clean(shape, mode)
    w = fm.Window(L, N, M, mode == "correlate")
    for c0, p in _nan_samples(w, C, N):
        assert 0 <= p < L
        xp = x.copy()
        xp[c0, p] = complex(np.nan, np.nan)
        _, yp = _fir_run(sm, xp, h, N, mode)
        expect = np.zeros(L, bool)
        for s in range(w.segments()):
            if w.load_start(s) <= p < w.load_start(s) + N:
                b, e = w.store_window(s)
                expect[w.output_index(s, b):w.output_index(s, e)] = True
        assert expect.any()
        what = f"{_shape_id(shape)} {mode} NaN at x[{c0}, {p}]"
        for k in range(K):
            nan = np.isnan(yp[c0, k].real) | np.isnan(yp[c0, k].imag)
            assert np.array_equal(nan, expect), f"{what}: filter {k}: NaN outputs {np.nonzero(nan != expect)[0][:8].tolist()} differ from the loading windows"
        same = yp.view(np.uint64) == y.view(np.uint64)         # one word per complex64 element
        same[c0][:, expect] = True
        assert same.all(), f"{what}: outputs outside its windows changed: {np.argwhere(~same)[:4].tolist()}"


@pytest.mark.parametrize("mode", FIR_MODES)
@pytest.mark.parametrize("shape", FIR_SHAPES, ids=_shape_id)
def test_fir_nan_tap_reaches_exactly_its_filter(sm, fir_clean, shape, mode):
    """a NaN tap in a filter at a filter-group boundary (the first filter of the second group, or the last filter of the only one)"""
    N, C, L, K, M = shape
    x, h, spec, y = fir_clean(shape, mode)
    tiles = -(-fm.Window(L, N, M, False).segments() * C // (4096 // N))
    groups = max(1, min(K, -(-2048 // tiles)))         # smfft_fir.hpp fir_filter_group_size, as test_fir_gpu.py restates it
    size = -(-K // groups)
    k0 = size if size < K else K - 1
    hp = h.copy()
    hp[k0, M // 3] = complex(np.nan, np.nan)
    sp, yp = _fir_run(sm, x, hp, N, mode)
    what = f"{_shape_id(shape)} {mode} NaN tap in filter {k0}"
    assert np.isnan(sp[k0].view(np.float32)).all(), f"{what}: spectrum row not entirely NaN"
    others = np.arange(K) != k0
    assert np.array_equal(sp[others].view(np.uint32), spec[others].view(np.uint32)), f"{what}: other spectrum rows changed"
    assert np.isnan(yp[:, k0].view(np.float32)).all(), f"{what}: output rows of the filter not entirely NaN"
    assert np.array_equal(yp[:, others].view(np.uint32), y[:, others].view(np.uint32)), f"{what}: other filters' outputs changed"

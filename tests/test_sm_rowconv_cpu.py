"""CPU checks of the row-pair convolutions (smfft_amd/csrc/smfft_rowconv.hip, libsmfft_rowconv.so): the model's fp64 reference
(tools/rowconv_model.py `direct`) is np.convolve and np.correlate(..., 'full') and its window is a slice; the model's chain in fp64 is
that reference and in fp32 stays far inside the GPU tests' bounds; the model's and the library's fft_size agree over the whole grid; the
gfx950 code of the five kernels keeps the budget of the FIR bank's and the chirp-z kernels; and the C ABI declares, exports and
validates the four entry points without a device.  No GPU code is run (hipcc cross-compiles gfx950)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rowconv_model as rm  # noqa: E402

from tests import addon_checks as ac  # noqa: E402
from tests import rowconv_inventory  # noqa: E402

CSRC = ac.CSRC
LIB = os.path.join(ROOT, "smfft_amd", "libsmfft_rowconv.so")
SIZES = (256, 512, 1024, 2048, 4096)
NAMES = ("smfft_rowconv_fft_size", "smfft_rowconv_launch", "smfft_rowconv_launch_tuned", "smfft_rowconv_benchmark")
LDS_BUDGET = 34816             # 4096 / 16 * 17 float2: the transform region of 4096 points, what the FIR bank's kernels hold
NO_DEVICE = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
SMALL = ((1, 1), (1, 7), (7, 1), (5, 3), (3, 5), (16, 16), (33, 20), (128, 129), (200, 57))


@pytest.fixture(scope="module")
def rowconv_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", CSRC, "-j", "4", "../libsmfft_rowconv.so"])
    return LIB


def _rand(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# ---- 1: the model -------------------------------------------------------------------------------------------
def test_direct_is_numpys_convolve_and_correlate():
    """fp64, small shapes, both modes: within 1e-13 of the largest output (both are fp64 sums of at most 200 terms in other orders);
    correlate is the convolution with the reversed conjugate; the window is a slice of the full result"""
    rng = np.random.default_rng(20)
    for n_a, n_b in SMALL:
        a, b = _rand(rng, (3, n_a)), _rand(rng, (3, n_b))
        full = n_a + n_b - 1
        for correlate, numpy_form in ((False, np.convolve), (True, lambda u, v: np.correlate(u, v, "full"))):
            want = np.stack([numpy_form(a[r], b[r]) for r in range(3)])
            got = rm.direct(a, b, correlate)
            assert got.shape == want.shape == (3, full) and got.dtype == np.complex128
            err = np.max(np.abs(got - want)) / np.max(np.abs(want))
            print(f"n_a={n_a} n_b={n_b} correlate={correlate}: max |direct - numpy| / max |numpy| = {err:.2e}")
            assert err <= 1e-13, (n_a, n_b, correlate, err)
            for first, m in {(0, 1), (full - 1, 1), (0, full), (full // 2, full - full // 2), (full // 3, 1)}:
                assert np.array_equal(rm.direct(a, b, correlate, first, m), got[:, first:first + m]), (n_a, n_b, first, m)
        assert np.array_equal(rm.direct(a, b, True), rm.direct(a, np.conj(b[:, ::-1]), False))
    # lag k - (n_b - 1) sits at index k: an impulse pair
    a, b = np.zeros(6), np.zeros(4)
    a[4], b[1] = 1, 1
    assert int(np.argmax(np.abs(rm.direct(a, b, True)))) == (4 - 1) + (4 - 1)
    assert int(np.argmax(np.abs(rm.direct(a, b, False)))) == 4 + 1
    for bad in ((-1, 1), (0, 0), (3, 6), (0, 9)):
        with pytest.raises(ValueError):
            rm.direct(np.ones(5), np.ones(4), False, *bad)


def test_model_chain_is_direct_and_its_fp32_form_is_inside_the_bounds():
    """the chain pad, FFT_M, product, IFFT_M, window: in fp64 within 1e-12 of the largest output of `direct`, in fp32 per row within a
    third of the bounds the GPU tests hold the kernel to (ROW_REL_L2 = 1e-6, ROW_MAX = 5e-6), both modes, on both sides of M boundaries"""
    rng = np.random.default_rng(21)
    for n_a, n_b in ((1, 1), (1, 256), (128, 129), (129, 129), (200, 57), (1000, 25), (1000, 26), (2048, 2049), (4095, 2), (1, 4096), (3, 4094)):
        a, b = _rand(rng, (3, n_a)).astype(np.complex64), _rand(rng, (3, n_b)).astype(np.complex64)
        for correlate in (False, True):
            want = rm.direct(a, b, correlate)
            err = np.max(np.abs(rm.model(a, b, correlate) - want)) / np.max(np.abs(want))
            d = rm.model(a, b, correlate, dtype=np.complex64) - want
            l2 = np.max(np.linalg.norm(d, axis=1) / np.linalg.norm(want, axis=1))
            mx = np.max(np.max(np.abs(d), axis=1) / np.max(np.abs(want), axis=1))
            print(f"n_a={n_a} n_b={n_b} correlate={correlate}: fp64 chain {err:.2e}; fp32 chain relL2 = {l2:.2e}, max |d| / max |want| = {mx:.2e}")
            assert err <= 1e-12 and l2 <= 1e-6 / 3 and mx <= 5e-6 / 3, (n_a, n_b, correlate, err, l2, mx)
            full = n_a + n_b - 1
            assert np.array_equal(rm.model(a, b, correlate, full // 2, 1), rm.model(a, b, correlate)[:, full // 2:full // 2 + 1])


def _want_sizes(count):
    """(count x count) of the minimal M over 1 <= n_a, n_b <= count, -1 where n_a + n_b - 1 > 4096"""
    n = np.arange(1, count + 1)
    need = n[:, None] + n[None, :] - 1
    want = np.full(need.shape, 256)
    for M in SIZES[1:]:
        want[need > M // 2] = M
    want[need > 4096] = -1
    return need, want


def test_fft_size_is_minimal_and_symmetric():
    need, want = _want_sizes(4097)
    ok = want > 0
    assert np.all(want[ok] >= need[ok]) and np.all((want[ok] == 256) | (want[ok] // 2 < need[ok])) and np.array_equal(want, want.T)
    assert np.array_equal(ok, need <= 4096)
    for i in (1, 2, 127, 128, 129, 1000, 2048, 2049, 4095, 4096):          # whole rows of the grid through the model ...
        for j in range(1, 4098):
            if want[i - 1, j - 1] > 0:
                assert rm.fft_size(i, j) == rm.fft_size(j, i) == want[i - 1, j - 1], (i, j)
            else:
                with pytest.raises(ValueError):
                    rm.fft_size(i, j)
    for bad in ((0, 5), (5, 0), (-1, 5), (4097, 1), (1, 4097), (2049, 2049)):
        with pytest.raises(ValueError):
            rm.fft_size(*bad)
    for M, shapes in rowconv_inventory.SHAPES.items():
        assert all(rm.fft_size(*s) == M for s in shapes), M


def test_library_fft_size_over_the_whole_grid(rowconv_lib, tmp_path):
    """... and the library's own over all 4097 x 4097 shapes, in a process with no visible device: the model's M, -1 where the model
    refuses"""
    code = r"""
import ctypes, sys
import numpy as np
lib = ctypes.CDLL(sys.argv[1])
f = lib.smfft_rowconv_fft_size
got = np.array([[f(n_a, n_b) for n_b in range(1, 4098)] for n_a in range(1, 4098)], np.int32)
np.save(sys.argv[2], got)
bad = [f(n_a, n_b) for n_a, n_b in ((0, 5), (5, 0), (-1, 5), (5, -1), (4097, 1), (1, 4097), (2049, 2049), (2**31 - 1, 2**31 - 1), (2**31 - 1, 2), (-2**31, 5))]
sys.exit(0 if bad == [-1] * len(bad) and f(300, 200) == 512 and f(4096, 1) == 4096 and f(2048, 2049) == 4096 else 1)
"""
    path = str(tmp_path / "sizes.npy")
    p = subprocess.run([sys.executable, "-c", code, rowconv_lib, path], capture_output=True, text=True, timeout=600, env=dict(os.environ, **NO_DEVICE))
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.load(path)
    need, want = _want_sizes(4097)
    assert np.array_equal(got, want) and np.array_equal(got, got.T)
    for i in (1, 128, 2048, 4096):
        assert [rm.fft_size(i, j) for j in range(1, 4098 - i)] == list(got[i - 1, :4097 - i]), i


# ---- 2: ISA budget and inventory -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """{M: assembly of smfft_rowconv_<M>.o as the Makefile compiles it}"""
    if not os.path.exists(ac.HIPCC):
        pytest.skip("hipcc not installed")
    return ac.addon_isa("smfft_rowconv", "ROWCONV", SIZES, tmp_path_factory.mktemp("rowconv_isa"))


def test_isa_budget_of_what_ships(isa):
    """per M exactly one kernel, read from the compiled object's metadata: no scratch, at most 256 VGPRs (two waves per SIMD), static LDS
    at most 34,816 B (the transform region of 4096 points and nothing else: there are no tables), no transcendentals, no packed f32
    arithmetic; a thread's 32 row loads -- the kernel's only non-temporal loads -- go out up front with no branch, barrier or vmcnt(0)
    wait between the first and the last, and every wait among them leaves at least ten in flight; the sixteen stores are non-temporal
    and follow them"""
    total = 0
    for m, text in isa.items():
        descs = ac.descriptors(text)
        kernels = ac.pfb_kernels(text, "rowconv_kernel")
        assert len(descs) == 1 and set(descs) == set(kernels), (m, sorted(descs))
        total += len(descs)
        assert not re.search(r"\bscratch_", text), m
        (name, body), = kernels.items()
        assert "rowconv_kernelILi%dE" % m in name
        assert not [line for line in body if re.match(r"v_(sin|cos)_", line)], name
        assert not [line for line in body if re.match(r"v_pk_(add|mul|fma)_f32", line)], name
        assert ac.descriptor_field(descs, name, "private_segment_fixed_size") == 0, name
        v, lds = ac.descriptor_field(descs, name, "next_free_vgpr"), ac.descriptor_field(descs, name, "group_segment_fixed_size")
        print(f"M={m}: rowconv_kernel {v} VGPRs ({ac.occupancy(v)} waves per SIMD), {lds} B of LDS, 0 B of scratch")
        assert lds <= LDS_BUDGET and 2 * lds <= ac.LDS_PER_CU, (name, lds)
        assert v <= 256 and ac.occupancy(v) >= 2, (name, v)
        loads = [i for i, line in enumerate(body) if line.startswith("global_load") and re.search(r"\bnt\b", line)]
        assert len(loads) == 32 and all(re.match(r"global_load_dwordx2\s", body[i]) for i in loads), (name, len(loads))
        between = body[loads[0]:loads[-1] + 1]
        assert not [line for line in between if line.startswith(("s_cbranch", "s_branch", "s_setpc", "s_barrier"))], name
        waits = [int(w) for line in between for w in re.findall(r"vmcnt\((\d+)\)", line)]
        assert all(w >= 10 for w in waits), (name, waits)
        stores = [i for i, line in enumerate(body) if line.startswith("global_store")]
        assert len(stores) == 16 and all(re.match(r"global_store_dwordx2\s", body[i]) and re.search(r"\bnt\b", body[i]) for i in stores), (name, len(stores))
        assert min(stores) > max(loads), name
    assert total == 5


def test_library_ships_five_kernels_and_the_inventory_names_them(rowconv_lib):
    ac.check_inventory(rowconv_lib, rowconv_inventory.KERNELS, "smfft_rowconv_", 5, kinds=("tests", "bounds", "probes"))
    assert "permlane" in rowconv_inventory.__doc__ and "hostsim" in rowconv_inventory.__doc__


def test_isa_identity_compares_the_library():
    """tools/isa_identity.py compiles the five objects with the Makefile's flags and -I., like the other add-ons' (the tool itself
    needs the history of a git checkout and minutes of compiling: it is run by hand, DESIGN.md section 20 has its verdict)"""
    ac.check_isa_identity_lists("smfft_rowconv", "ROWCONV", SIZES)


# ---- 3: declarations and exports ---------------------------------------------------------------------------------
def test_python_mirror_matches_header(rowconv_lib):
    from smfft_amd import rowconv
    header = re.sub(r"[\s*]+", " ", open(os.path.join(ROOT, "include", "smfft_rowconv.h")).read())
    for phrase in ("Rows are float2. Row r of a is at element r n_a. Row r of b is at element r n_b. Row r of the output is at element r m. "
                   "All offsets are 64-bit. Let Lfull = n_a + n_b - 1.",
                   "y[r][k] = sum_j a[r][j] b[r][k - j] for 0 <= k < Lfull", "This is np.convolve(a[r], b[r]).",
                   "y[r][k] = sum_j a[r][j + k - (n_b - 1)] conj(b[r][j])", "This is np.correlate(a[r], b[r], 'full'), so lag k - (n_b - 1) sits at index k.",
                   "np.convolve(a[r], conj(b[r][::-1]))", "out[r m + i] = y[r][first + i] for 0 <= i < m, with 0 <= first, 1 <= m and first + m <= Lfull",
                   "Out of scope", "real rows (two real rows in one complex transform need a Hermitian split across threads)",
                   "Lfull > 4096 (that is the large engine's ground)", "one b shared by all rows (that is smfft_fir_ )",
                   "a peak / arg-max output over the lags", "shrinking M for narrow windows", "strided rows",
                   "d_a == d_b is allowed", "every output element is written exactly once", "Rows do not see each other",
                   "only a[0, batch n_a), b[0, batch n_b) and out[0, batch m) are touched", "8-byte alignment",
                   "batch == 0 launches nothing and returns 0"):
        assert phrase in header, phrase
    decl = ac.declarations("smfft_rowconv.h")
    assert sorted(decl) == sorted(rowconv.SIGS) == sorted(NAMES)
    for name, (res, args) in decl.items():
        assert rowconv.SIGS[name] == ac.signature(res, args), name
    sigs = rowconv.SIGS
    # launch_tuned = the arguments of launch + grid; benchmark = launch with the timer in the stream's place
    assert sigs["smfft_rowconv_launch_tuned"][1] == sigs["smfft_rowconv_launch"][1] + [ac.CTYPES["int"]]
    assert sigs["smfft_rowconv_benchmark"][1] == sigs["smfft_rowconv_launch"][1][:-1] + [ac.CTYPES["double*"]]
    assert rowconv.SIZES == SIZES and rowconv.MAX_FULL == 4096


def test_library_exports_exactly_the_four_symbols(rowconv_lib):
    ac.check_exports(rowconv_lib, NAMES)


# ---- 4: rejections -------------------------------------------------------------------------------------------------
def test_unsupported_combinations_return_minus_one_without_a_device(rowconv_lib):
    """-1 (or 0 for an empty batch) before any HIP call: run in a process where no GPU is visible, with addresses that are never read.
    d_out == d_a and d_out == d_b are refused whatever the batch; d_a == d_b is not"""
    code = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
ll, d, vp, i = ctypes.c_longlong, ctypes.c_double, ctypes.c_void_p, ctypes.c_int
head = [vp, vp, vp, i, i, i, i, ll, i]
lib.smfft_rowconv_launch.argtypes = head + [vp]
lib.smfft_rowconv_launch_tuned.argtypes = head + [vp, i]
lib.smfft_rowconv_benchmark.argtypes = head + [ctypes.POINTER(d)]
t = d(0.0)
A, B, OUT = 4096, 8192, 16384
def calls(n_a, n_b, first, m, batch, grid=3, da=A, db=B, dout=OUT):
    out = []
    for c in (0, 1, 7):
        out += [lib.smfft_rowconv_launch(da, db, dout, n_a, n_b, first, m, batch, c, None),
                lib.smfft_rowconv_launch_tuned(da, db, dout, n_a, n_b, first, m, batch, c, None, grid),
                lib.smfft_rowconv_benchmark(da, db, dout, n_a, n_b, first, m, batch, c, ctypes.byref(t))]
    return out
rc = []
# sizes outside the range
for n_a, n_b in ((0, 5), (5, 0), (-5, 5), (5, -5), (4097, 1), (1, 4097), (2049, 2049), (4096, 2), (2**31 - 1, 2**31 - 1), (2**31 - 1, 3)):
    rc += calls(n_a, n_b, 0, 1, 10) + calls(n_a, n_b, 0, 1, 0) + [lib.smfft_rowconv_fft_size(n_a, n_b)]
# windows outside the full result of (300, 200): Lfull = 499
for first, m in ((-1, 5), (0, 0), (0, -3), (0, 500), (1, 499), (499, 1), (498, 2), (2**31 - 1, 1), (1, 2**31 - 1), (2**31 - 1, 2**31 - 1)):
    rc += calls(300, 200, first, m, 10) + calls(300, 200, first, m, 0)
# batch < 0; grid < 1, for an empty batch too
for n_a, n_b in ((1, 1), (300, 200), (2048, 2049), (4096, 1)):
    rc += calls(n_a, n_b, 0, 1, -1)
    for grid in (0, -1):
        rc += [lib.smfft_rowconv_launch_tuned(A, B, OUT, n_a, n_b, 0, 1, batch, 0, None, grid) for batch in (10, 0)]
# the output is an input: refused, for an empty batch and for null == null too
for n_a, n_b in ((300, 200), (1, 1), (2048, 2048)):
    for batch in (10, 0):
        rc += calls(n_a, n_b, 0, 1, batch, dout=A) + calls(n_a, n_b, 0, 1, batch, dout=B) + calls(n_a, n_b, 0, 1, batch, da=A, db=A, dout=A)
        rc += calls(n_a, n_b, 0, 1, batch, da=None, db=None, dout=None) + calls(n_a, n_b, 0, 1, batch, da=None, dout=None) + calls(n_a, n_b, 0, 1, batch, db=None, dout=None)
empty = []
for n_a, n_b, first, m in ((1, 1, 0, 1), (300, 200, 0, 499), (300, 200, 498, 1), (2048, 2049, 2045, 7), (4096, 1, 0, 4096), (1, 4096, 4095, 1)):
    empty += calls(n_a, n_b, first, m, 0) + calls(n_a, n_b, first, m, 0, da=A, db=A)             # d_a == d_b is allowed
print(rc, empty, t.value)
sys.exit(0 if rc and rc == [-1] * len(rc) and empty == [0] * 108 and t.value == 0.0 else 1)
"""
    p = subprocess.run([sys.executable, "-c", code, rowconv_lib], capture_output=True, text=True, timeout=120, env=dict(os.environ, **NO_DEVICE))
    assert p.returncode == 0, p.stdout + p.stderr


def test_python_wrappers_refuse_before_a_device(rowconv_lib):
    from smfft_amd import rowconv
    A, B, OUT = 4096, 8192, 16384
    for n_a, n_b in ((0, 5), (5, 0), (-5, 5), (4097, 1), (1, 4097), (2049, 2049)):
        with pytest.raises(RuntimeError):
            rowconv.launch(A, B, OUT, n_a, n_b, 0, 1, 10)
        with pytest.raises(RuntimeError):
            rowconv.launch_tuned(A, B, OUT, n_a, n_b, 0, 1, 10, 3)
        assert rowconv.benchmark(A, B, OUT, n_a, n_b, 0, 1, 10) == (-1, 0.0)
        with pytest.raises(ValueError):
            rowconv.fft_size(n_a, n_b)
    for first, m in ((-1, 5), (0, 0), (0, 500), (499, 1), (498, 2)):
        with pytest.raises(RuntimeError):
            rowconv.launch(A, B, OUT, 300, 200, first, m, 10, correlate=True)
        with pytest.raises(ValueError):
            rowconv.convolve(np.zeros(300), np.zeros(200), first=first, m=m)
    with pytest.raises(RuntimeError):
        rowconv.launch(A, B, OUT, 300, 200, 0, 499, -1)
    for dout in (A, B):
        for batch in (10, 0):                                        # the output is an input: refused for an empty batch too
            with pytest.raises(RuntimeError):
                rowconv.launch(A, B, dout, 300, 200, 0, 499, batch)
            with pytest.raises(RuntimeError):
                rowconv.launch_tuned(A, B, dout, 300, 200, 0, 499, batch, 3)
            assert rowconv.benchmark(A, B, dout, 300, 200, 0, 499, batch) == (-1, 0.0)
    for grid in (0, -1):
        with pytest.raises(RuntimeError):
            rowconv.launch_tuned(A, B, OUT, 300, 200, 0, 499, 10, grid)
    rowconv.launch(A, A, OUT, 300, 300, 0, 599, 0, correlate=True)   # d_a == d_b, an empty batch: nothing is launched
    assert rowconv.benchmark(A, B, OUT, 300, 200, 0, 499, 0) == (0, 0.0)
    with pytest.raises(ValueError):
        rowconv.convolve(np.zeros(4096, np.complex64), np.zeros(2, np.complex64))
    with pytest.raises(ValueError):
        rowconv.convolve(np.zeros((3, 0), np.complex64), np.zeros((3, 5), np.complex64))
    with pytest.raises(ValueError):
        rowconv.convolve(np.zeros((3, 5), np.complex64), np.zeros((2, 5), np.complex64))     # rows do not pair
    with pytest.raises(ValueError):
        rowconv.convolve(np.complex64(1), np.zeros(5, np.complex64))
    assert rowconv.fft_size(300, 200) == 512


def test_import_does_not_load_the_library():
    ac.check_import_does_not_load("rowconv", "smfft_rowconv")

"""CPU checks of the DCT / DST library (smfft_amd/csrc/smfft_dct.hip, libsmfft_dct.so): the model's chain (tools/dct_model.py) in fp64
is the fp64 sum of the definition for all four transforms, and in fp32 stays inside the GPU tests' bounds; the generated twiddle octant
is the committed one and its symmetries give fp64 values rounded once; the gfx950 code of the ten kernels keeps its budget; and the C
ABI declares, exports and validates the four entry points without a device.  No GPU code is run (hipcc cross-compiles gfx950)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dct_model as dm  # noqa: E402
import gen_twiddles_dct  # noqa: E402

from tests import addon_checks as ac  # noqa: E402
from tests import dct_inventory  # noqa: E402
from tests.fir_gpu_harness import ROW_MAX, ROW_REL_L2  # noqa: E402

CSRC = ac.CSRC
LIB = os.path.join(ROOT, "smfft_amd", "libsmfft_dct.so")
SIZES = (256, 512, 1024, 2048, 4096)
LENGTHS = (512, 1024, 2048, 4096, 8192)
NAMES = ("smfft_dct_fft_size", "smfft_dct_launch", "smfft_dct_launch_tuned", "smfft_dct_benchmark")
TRANSFORMS = ((2, False), (3, False), (2, True), (3, True))
LDS_BUDGET = 34816             # 4096 / 16 * 17 float2: the transform region of 4096 points; the kernels have no other LDS
NO_DEVICE = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


@pytest.fixture(scope="module")
def dct_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", CSRC, "-j", "4", "../libsmfft_dct.so"])
    return LIB


def _rows(rng, shape):
    return rng.standard_normal(shape).astype(np.float32)


# ---- 1: the model -------------------------------------------------------------------------------------------
def test_fp64_chain_is_the_direct_sums_and_the_dst_identities_hold():
    """n = 512, three Gaussian rows: the chain in fp64 within 1e-12 relL2 of the cosine and sine sums of the definition for the four
    transforms; DST-II(x)[k] = DCT-II(s x)[n - 1 - k] and DST-III(X)[j] = s_j DCT-III(reverse X)[j] with s_j = (-1)^j; type III undoes
    type II up to 2n; float64 out"""
    n = 512
    x = _rows(np.random.default_rng(220), (3, n))
    s = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    for type, sine in TRANSFORMS:
        want, got = dm.direct(x, type, sine), dm.chain(x, type, sine)
        assert got.shape == x.shape and got.dtype == np.float64
        l2, mx = dm.errors(got, want)
        print(f"type {type} sine {sine}: fp64 chain relL2 = {l2:.2e}, max = {mx:.2e}")
        assert l2 <= 1e-12 and mx <= 1e-12, (type, sine, l2, mx)
    assert dm.errors(dm.direct(x, 2, True), dm.direct(s * x, 2, False)[:, ::-1])[0] <= 1e-13
    assert dm.errors(dm.direct(x, 3, True), s * dm.direct(x[:, ::-1], 3, False))[0] <= 1e-13
    for sine in (False, True):
        assert dm.errors(dm.direct(dm.direct(x, 2, sine), 3, sine) / (2 * n), x)[0] <= 1e-12
    with pytest.raises(ValueError):
        dm.chain(np.zeros(500), 2)
    with pytest.raises(ValueError):
        dm.chain(np.zeros(512), 4)


def test_fp64_chain_is_scipys():
    """scipy.fft.dct / dst with norm=None, types 2 and 3, at n = 512 and 8192"""
    sf = pytest.importorskip("scipy.fft")
    for n in (512, 8192):
        x = _rows(np.random.default_rng(221 + n), (2, n))
        for type, sine in TRANSFORMS:
            want = (sf.dst if sine else sf.dct)(x.astype(np.float64), type=type, axis=-1)
            l2, mx = dm.errors(dm.chain(x, type, sine), want)
            assert l2 <= 1e-12 and mx <= 1e-12, (n, type, sine, l2, mx)


def test_fp32_model_is_inside_the_bounds():
    """every stage of the chain rounded to fp32 (the transform itself in fp64, rounded once), n = 512 and 8192, the four transforms: the
    row bounds of the GPU tests hold.  Beside it the same model with W_4n from angles rounded to fp32 first (sinf-grade values) is
    printed, without asserting which way it falls"""
    worst = [0.0, 0.0]
    for n in (512, 8192):
        x = _rows(np.random.default_rng(222 + n), (3, n))
        for type, sine in TRANSFORMS:
            want = dm.chain(x, type, sine)
            l2, mx = dm.errors(dm.chain(x, type, sine, np.float32), want)
            fl2, fmx = dm.errors(dm.chain(x, type, sine, np.float32, fast_w4=True), want)
            print(f"n={n} type {type} sine {sine}: fp32 model relL2 = {l2:.2e}, max = {mx:.2e}; with fast W_4n {fl2:.2e}, {fmx:.2e}")
            worst = [max(worst[0], l2), max(worst[1], mx)]
            assert l2 <= ROW_REL_L2 and mx <= ROW_MAX, (n, type, sine, l2, mx)
    print(f"fp32 model, worst: relL2 = {worst[0]:.2e}, max |d| / max |want| = {worst[1]:.2e}")
    assert ROW_REL_L2 == 1e-6 and ROW_MAX == 5e-6


def test_pack_index_is_the_permutation():
    """z[p] = v[2p] + i v[2p + 1] with v[j] = x[2j], v[n - 1 - j] = x[2j + 1]: the two index rows cover every sample once"""
    for n in LENGTHS:
        v = np.empty(n, np.int64)
        v[:n // 2] = np.arange(0, n, 2)
        v[n - 1 - np.arange(n // 2)] = np.arange(1, n, 2)
        i0, i1 = dm.pack_index(n)
        assert np.array_equal(i0, v[0::2]) and np.array_equal(i1, v[1::2])
        assert np.array_equal(np.sort(np.concatenate([i0, i1])), np.arange(n))


def test_twiddle_octant_is_the_generated_one():
    """the committed table is the generator's text; the symmetries that the kernels' compile-time rows apply give, over the whole half
    circle, values within half an ulp of one of fp64's (2^-25, with one per cent for the second rounding of the mirrored entries), and
    exactly 1 and 0 where the sines and cosines are"""
    path = os.path.join(ROOT, "include", "smfft", "smfft_twiddles_dct.inc")
    assert os.path.abspath(gen_twiddles_dct.PATH) == os.path.abspath(path)
    assert open(path).read() == gen_twiddles_dct.table_text()
    c, s = gen_twiddles_dct.full_table()
    ang = 2 * np.pi * np.arange(16384) / 32768
    assert np.max(np.abs(c.astype(np.float64) - np.cos(ang))) <= 1.01 * 2.0 ** -25
    assert np.max(np.abs(s.astype(np.float64) - np.sin(ang))) <= 1.01 * 2.0 ** -25
    assert c[0] == 1 and s[0] == 0 and c[8192] == 0 and s[8192] == 1 and c[4096] == s[4096]
    # the table and its symmetries live in the header that the four half-length row libraries share
    source = open(os.path.join(CSRC, "smfft_rows.hpp")).read()
    assert "smfft/smfft_twiddles_dct.inc" in source and "b.y, b.x" in source and "-a.y, a.x" in source and "-b.x, b.y" in source
    assert '#include "smfft_rows.hpp"' in open(os.path.join(CSRC, "smfft_dct.hip")).read()


# ---- 2: ISA budget and inventory -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """{M: assembly of smfft_dct_<M>.o as the Makefile compiles it}"""
    if not os.path.exists(ac.HIPCC):
        pytest.skip("hipcc not installed")
    return ac.addon_isa("smfft_dct", "DCT", SIZES, tmp_path_factory.mktemp("dct_isa"))


def test_isa_budget_of_what_ships(isa):
    """per M exactly the two kernels, read from the compiled object's metadata: no scratch, at most 256 VGPRs (two waves per SIMD),
    static LDS of exactly 34,816 B (the transform region of 4096 points: no table in LDS), no transcendentals, no packed f32 arithmetic;
    a thread's row loads -- eight 16-byte non-temporal ones (type II) or thirty-two plain 4-byte ones (type III) -- go out up front with
    no branch or barrier between the first and the last, and the stores -- thirty-two plain 4-byte ones (type II) or eight 16-byte
    non-temporal ones (type III; plain at M = 2048, where the Makefile's flag says so) -- follow them"""
    total = 0
    for m, text in isa.items():
        descs = ac.descriptors(text)
        kernels = {**ac.pfb_kernels(text, "dct2_kernel"), **ac.pfb_kernels(text, "dct3_kernel")}
        assert len(descs) == 2 and set(descs) == set(kernels), (m, sorted(descs))
        total += len(descs)
        assert not re.search(r"\bscratch_", text), m
        for name, body in kernels.items():
            assert re.search(r"dct[23]_kernelILi%dE" % m, name)
            assert not [line for line in body if re.match(r"v_(sin|cos)_", line)], name
            assert not [line for line in body if re.match(r"v_pk_(add|mul|fma)_f32", line)], name
            assert ac.descriptor_field(descs, name, "private_segment_fixed_size") == 0, name
            v, lds = ac.descriptor_field(descs, name, "next_free_vgpr"), ac.descriptor_field(descs, name, "group_segment_fixed_size")
            print(f"M={m}: {'dct2_kernel' if 'dct2' in name else 'dct3_kernel'} {v} VGPRs ({ac.occupancy(v)} waves per SIMD), {lds} B of LDS, 0 B of scratch")
            assert lds == LDS_BUDGET and 2 * lds <= ac.LDS_PER_CU, (name, lds)
            assert v <= 256 and ac.occupancy(v) >= 2, (name, v)
            # the row accesses: type II loads and type III stores eight 16-byte quads per thread, non-temporal (but for type III's at
            # M = 2048); type II stores and type III loads thirty-two floats, plain (the other loads, 8 bytes each, are twiddles)
            two = "dct2" in name
            loads = [i for i, line in enumerate(body) if re.match(r"global_load_dwordx4\s" if two else r"global_load_dword\s", line)]
            stores = [i for i, line in enumerate(body) if line.startswith("global_store")]
            assert len(loads) == (8 if two else 32) and len(stores) == (32 if two else 8), (name, len(loads), len(stores))
            assert all(bool(re.search(r"\bnt\b", body[i])) == two for i in loads), name
            quads_nt = "-DSMFFT_DCT_NT_STORE4=0" not in ac.makefile_flags("DCT", m)          # (plain at M = 2048: the Makefile says why)
            assert quads_nt == (m != 2048)
            assert all(re.match(r"global_store_dword\s" if two else r"global_store_dwordx4\s", body[i])
                       and bool(re.search(r"\bnt\b", body[i])) == (not two and quads_nt) for i in stores), name
            assert len([line for line in body if line.startswith("global_load") and re.search(r"\bnt\b", line)]) == (8 if two else 0), name
            between = body[loads[0]:loads[-1] + 1]
            assert not [line for line in between if line.startswith(("s_cbranch", "s_branch", "s_setpc", "s_barrier"))], name
            assert min(stores) > max(loads), name
    assert total == 10


def test_library_ships_ten_kernels_and_the_inventory_names_them(dct_lib):
    ac.check_inventory(dct_lib, dct_inventory.KERNELS, "smfft_dct_", 10, kinds=("tests", "bounds", "probes"))
    assert "permlane" in dct_inventory.__doc__ and "hostsim" in dct_inventory.__doc__


def test_isa_identity_compares_the_library():
    """tools/isa_identity.py compiles the five objects with the Makefile's flags and -I., like the other add-ons' (the tool itself
    needs the history of a git checkout and minutes of compiling: it is run by hand, DESIGN.md section 22 has its verdict)"""
    ac.check_isa_identity_lists("smfft_dct", "DCT", SIZES)


# ---- 3: declarations and exports ---------------------------------------------------------------------------------
def test_python_mirror_matches_header(dct_lib):
    from smfft_amd import dct
    header = re.sub(r"[\s*]+", " ", open(os.path.join(ROOT, "include", "smfft_dct.h")).read())
    for phrase in ("Un-normalised, the convention of scipy.fft with norm=None", "X[k] = 2 sum_j x[j] cos(pi k (2j+1) / (2n))",
                   "y[j] = X[0] + 2 sum_{k>=1} X[k] cos(pi k (2j+1) / (2n))", "X[k] = 2 sum_j x[j] sin(pi (k+1)(2j+1) / (2n))",
                   "y[j] = (-1)^j X[n-1] + 2 sum_{k<n-1} X[k] sin(pi (k+1)(2j+1) / (2n))", "DCT-III(DCT-II(x)) = 2n x",
                   "In place, d_out == d_in, is allowed", "Ranges that overlap without being equal are refused", "4-byte alignment",
                   "every output element is written exactly once", "the bits of row r's outputs depend only on x[r], n, type and sine",
                   "A NaN or Inf in a row stays in that row", "batch == 0 launches nothing and returns 0", "Out of scope",
                   "n < 512, n > 8192 and n that is not a power of two", "types I and IV", "orthonormal scaling", "two-dimensional transforms"):
        assert phrase in header, phrase
    decl = ac.declarations("smfft_dct.h")
    assert sorted(decl) == sorted(dct.SIGS) == sorted(NAMES)
    for name, (res, args) in decl.items():
        assert dct.SIGS[name] == ac.signature(res, args), name
    assert dct.SIZES == SIZES and dct.LENGTHS == LENGTHS and dct.TYPES == (2, 3)


def test_library_exports_exactly_the_four_symbols(dct_lib):
    ac.check_exports(dct_lib, NAMES)


# ---- 4: rejections -------------------------------------------------------------------------------------------------
def test_unsupported_combinations_return_minus_one_without_a_device(dct_lib):
    """-1 (or 0 for an empty batch) before any HIP call: run in a process where no GPU is visible, with addresses that are never read.
    Every length next to the five, types 1 and 4, batch < 0, overlapping unequal buffers, grid < 1"""
    code = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
ll, d, vp, i = ctypes.c_longlong, ctypes.c_double, ctypes.c_void_p, ctypes.c_int
head = [vp, vp, i, ll, i, i]
lib.smfft_dct_launch.argtypes = head + [vp]
lib.smfft_dct_launch_tuned.argtypes = head + [vp, i]
lib.smfft_dct_benchmark.argtypes = head + [ctypes.POINTER(d)]
t = d(0.0)
IN, OUT = 1 << 20, 1 << 30
def calls(n, batch, type, grid=3, din=IN, dout=OUT):
    out = []
    for s in (0, 1, 7):
        out += [lib.smfft_dct_launch(din, dout, n, batch, type, s, None),
                lib.smfft_dct_launch_tuned(din, dout, n, batch, type, s, None, grid),
                lib.smfft_dct_benchmark(din, dout, n, batch, type, s, ctypes.byref(t))]
    return out
rc = []
for n in (256, 500, 16384, 0, -512, 513, 1000, 8191, 2**31 - 1):
    for type in (2, 3):
        rc += calls(n, 10, type) + calls(n, 0, type) + calls(n, 10, type, dout=IN)
    rc += [lib.smfft_dct_fft_size(n)]
for n in (512, 8192):
    for type in (1, 4, 0, -2):
        rc += calls(n, 10, type) + calls(n, 0, type)
    for type in (2, 3):
        rc += calls(n, -1, type) + calls(n, -2**40, type)
        # overlapping, unequal: the output starts inside the input, ends inside it, or one element off
        for off in (4, 4 * n, 4 * (10 * n - 1), -4, -4 * (10 * n - 1)):
            rc += calls(n, 10, type, dout=IN + off)
        for grid in (0, -1):
            rc += [lib.smfft_dct_launch_tuned(IN, OUT, n, batch, type, 0, None, grid) for batch in (10, 0)]
            rc += [lib.smfft_dct_launch_tuned(IN, IN, n, batch, type, 0, None, grid) for batch in (10, 0)]
empty = []
for n in (512, 1024, 2048, 4096, 8192):
    for type in (2, 3):
        empty += calls(n, 0, type) + calls(n, 0, type, dout=IN) + calls(n, 0, type, dout=IN + 4) + calls(n, 0, type, din=None, dout=None)
sizes = [lib.smfft_dct_fft_size(n) for n in (512, 1024, 2048, 4096, 8192)]
print(rc, empty, t.value, sizes)
sys.exit(0 if rc and rc == [-1] * len(rc) and empty == [0] * 360 and t.value == 0.0 and sizes == [256, 512, 1024, 2048, 4096] else 1)
"""
    p = subprocess.run([sys.executable, "-c", code, dct_lib], capture_output=True, text=True, timeout=120, env=dict(os.environ, **NO_DEVICE))
    assert p.returncode == 0, p.stdout + p.stderr


def test_python_wrappers_refuse_before_a_device(dct_lib):
    """in a process where no GPU is visible: the pointer forms turn the library's -1 into a RuntimeError, the array forms raise
    ValueError or TypeError themselves, and an empty batch is served"""
    code = ac.REFUSED + r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from smfft_amd import dct
IN, OUT = 1 << 20, 1 << 30
for n in (256, 500, 16384, 0):
    refused(RuntimeError, dct.launch_ptr, IN, OUT, n, 10)
    refused(RuntimeError, dct.launch_tuned, IN, OUT, n, 10, 3)
    assert dct.benchmark(IN, OUT, n, 10) == (-1, 0.0)
    refused(ValueError, dct.fft_size, n)
    refused(ValueError, dct.dct, np.zeros((2, n), np.float32))
    refused(ValueError, dct.dst, np.zeros((2, n), np.float32), type=3)
for type in (1, 4):
    refused(RuntimeError, dct.launch_ptr, IN, OUT, 512, 10, type)
    refused(ValueError, dct.dct, np.zeros((2, 512), np.float32), type=type)
refused(RuntimeError, dct.launch_ptr, IN, OUT, 512, -1)
refused(RuntimeError, dct.launch_ptr, IN, IN + 4, 512, 10)
refused(RuntimeError, dct.launch_tuned, IN, OUT, 512, 10, 0)
refused(TypeError, dct.dct, np.zeros((2, 512), np.complex64))
refused(ValueError, dct.dct, np.float32(1))
refused(TypeError, dct.launch, np.zeros((2, 512), np.float32))
import torch
refused(ValueError, dct.launch, torch.zeros(2, 512))                     # a tensor on the host: no CPU fallback
refused(ValueError, dct.launch, torch.zeros(2, 500))
refused(TypeError, dct.launch, torch.zeros(2, 512, dtype=torch.float64))
refused(ValueError, dct.launch, torch.zeros(2, 1024)[:, ::2])
refused(ValueError, dct.launch, torch.zeros(2, 512), type=4)
dct.launch_ptr(IN, IN, 8192, 0, 3, True)                                  # an empty batch, in place: nothing is launched
assert dct.benchmark(IN, OUT, 512, 0) == (0, 0.0) and dct.fft_size(8192) == 4096
print("ok")
"""
    p = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300, env=dict(os.environ, **NO_DEVICE))
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout + p.stderr


def test_import_does_not_load_the_library():
    ac.check_import_does_not_load("dct", "smfft_dct")

"""CPU checks of the real row-pair convolutions (smfft_amd/csrc/smfft_rowconv_real.hip, libsmfft_rowconv_real.so): the model's chain
(tools/rowconv_real_model.py) in fp64 is the fp64 sum of the definition and in fp32, WITH the balancing of the two packed rows, stays
inside the GPU tests' bounds at every shape and scale, while without it it does not; the integer rule of the balancing
(smfft_rowconv_real_scale.hpp), compiled alone under the address and undefined-behaviour sanitizers, is the model's; the gfx950 code
of the five kernels keeps its budget; and the C ABI declares, exports and validates the four entry points without a device.  No GPU
code is run (hipcc cross-compiles gfx950)."""
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rowconv_real_model as rrm  # noqa: E402

from tests import addon_checks as ac  # noqa: E402
from tests import rowconv_real_inventory  # noqa: E402
from tests.fir_gpu_harness import ROW_MAX, ROW_REL_L2  # noqa: E402

CSRC = ac.CSRC
LIB = os.path.join(ROOT, "smfft_amd", "libsmfft_rowconv_real.so")
SIZES = (256, 512, 1024, 2048, 4096)
NAMES = ("smfft_rowconv_real_fft_size", "smfft_rowconv_real_launch", "smfft_rowconv_real_launch_tuned", "smfft_rowconv_real_benchmark")
LDS_BUDGET = 34816             # 4096 / 16 * 17 float2: the transform region of 4096 points
LDS_REDUCTION = 256            # ... plus at most this much for the row reductions across waves
NO_DEVICE = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
SHAPES = ((1, 1), (1, 256), (256, 1), (128, 129), (129, 129), (300, 200), (200, 300), (1000, 25), (1000, 26), (4095, 2), (2, 4095), (4096, 1),
          (1, 4096), (2048, 2049), (1536, 513))
SCALES = (-60, -12, 0, 12, 60)


@pytest.fixture(scope="module")
def real_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", CSRC, "-j", "4", "../libsmfft_rowconv_real.so"])
    return LIB


def _rows(rng, shape):
    return rng.standard_normal(shape).astype(np.float32)


# ---- 1: the model -------------------------------------------------------------------------------------------
def test_direct_is_numpys_convolve_and_correlate():
    """fp64, small shapes, both modes: np.convolve / np.correlate(..., 'full') within 1e-13 of the largest output; float64 out; the
    window is a slice; complex rows are refused"""
    rng = np.random.default_rng(210)
    for n_a, n_b in ((1, 1), (1, 7), (7, 1), (5, 3), (33, 20), (128, 129)):
        a, b = _rows(rng, (3, n_a)), _rows(rng, (3, n_b))
        full = n_a + n_b - 1
        for correlate, numpy_form in ((False, np.convolve), (True, lambda u, v: np.correlate(u, v, "full"))):
            want = np.stack([numpy_form(a[r].astype(np.float64), b[r].astype(np.float64)) for r in range(3)])
            got = rrm.direct(a, b, correlate)
            assert got.shape == (3, full) and got.dtype == np.float64
            assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want)), (n_a, n_b, correlate)
            assert np.array_equal(rrm.direct(a, b, correlate, full // 2, 1), got[:, full // 2:full // 2 + 1])
        assert np.array_equal(rrm.direct(a, b, True), rrm.direct(a, b[:, ::-1], False))
    with pytest.raises(TypeError):
        rrm.direct(np.ones(5, np.complex64), np.ones(4))
    assert rrm.fft_size(300, 200) == 512 and rrm.fft_size(2048, 2049) == 4096
    for M, shapes in rowconv_real_inventory.SHAPES.items():
        assert all(rrm.fft_size(*s) == M for s in shapes), M


def test_model_chain_in_fp64_is_direct():
    """pack, FFT_M, partner, product, IFFT_M, real part, window: within 1e-12 relL2 of `direct` per row, every shape, both modes, windows"""
    rng = np.random.default_rng(211)
    for n_a, n_b in SHAPES:
        a, b = _rows(rng, (3, n_a)), _rows(rng, (3, n_b))
        full = n_a + n_b - 1
        for correlate in (False, True):
            want = rrm.direct(a, b, correlate)
            l2, mx = rrm.errors(rrm.model(a, b, correlate), want)
            print(f"n_a={n_a} n_b={n_b} correlate={correlate}: fp64 chain relL2 = {l2:.2e}")
            assert l2 <= 1e-12, (n_a, n_b, correlate, l2)
            for first, m in {(0, 1), (full - 1, 1), (full // 2, full - full // 2)}:
                assert np.array_equal(rrm.model(a, b, correlate, first, m), rrm.model(a, b, correlate)[:, first:first + m])


def test_fp32_model_with_balancing_is_inside_the_bounds():
    """every stage rounded to fp32, b scaled by 2^s, s in -60, -12, 0, 12, 60: the row bounds of the GPU tests hold at every shape (the
    worst figures over all of them are printed: 1.4e-7 and 2.1e-7 when this was written)"""
    rng = np.random.default_rng(212)
    worst = [0.0, 0.0]
    for n_a, n_b in SHAPES:
        a, b0 = _rows(rng, (3, n_a)), _rows(rng, (3, n_b))
        for s in SCALES:
            b = np.ldexp(b0, s).astype(np.float32)
            for correlate in (False, True):
                l2, mx = rrm.errors(rrm.model(a, b, correlate, dtype=np.float32), rrm.direct(a, b, correlate))
                worst = [max(worst[0], l2), max(worst[1], mx)]
                assert l2 <= ROW_REL_L2 and mx <= ROW_MAX, (n_a, n_b, s, correlate, l2, mx)
    print(f"fp32 model with balancing, worst over {len(SHAPES)} shapes x {len(SCALES)} scales x 2 modes: relL2 = {worst[0]:.2e}, max |d| / max |want| = {worst[1]:.2e}")
    assert ROW_REL_L2 == 1e-6 and ROW_MAX == 5e-6


def test_fp32_model_without_balancing_breaks_the_bounds():
    """why step 2 of the kernel exists: the same chain without the row exponents misses the relL2 bound at (4096, 1), where the rows'
    energies differ by 2^12, and at (300, 200) with b scaled by 2^+-12"""
    rng = np.random.default_rng(213)
    for n_a, n_b, s in ((4096, 1, 0), (300, 200, 12), (300, 200, -12)):
        a, b = _rows(rng, (3, n_a)), np.ldexp(_rows(rng, (3, n_b)), s).astype(np.float32)
        want = rrm.direct(a, b, False)
        l2, mx = rrm.errors(rrm.model(a, b, False, dtype=np.float32, balance=False), want)
        good = rrm.errors(rrm.model(a, b, False, dtype=np.float32), want)
        print(f"n_a={n_a} n_b={n_b} b * 2^{s}: without balancing relL2 = {l2:.2e}, max = {mx:.2e}; with {good[0]:.2e}, {good[1]:.2e}")
        assert l2 > ROW_REL_L2 and good[0] <= ROW_REL_L2 and good[1] <= ROW_MAX, (n_a, n_b, s, l2, good)


def test_row_exponent_normalises_the_energy_and_model_handles_special_rows():
    """ldexp(x, k) has its sum of squares in [1, 4) for rows from 2^-140 to 2^120; zero rows give +0 bits, NaN and Inf rows NaN, row by row"""
    rng = np.random.default_rng(214)
    for n in (1, 2, 17, 4096):
        for s in (-140, -126, -60, 0, 1, 60, 120):
            x = np.ldexp(_rows(rng, (4, n)), s).astype(np.float32)
            k, zero, finite = rrm.row_exponent(x)
            energy = np.sum(np.ldexp(x.astype(np.float64), k[:, None]) ** 2, axis=1)
            assert not zero.any() and finite.all() and np.all((energy >= 1 - 1e-6) & (energy < 4 * (1 + 1e-6))), (n, s, energy)
    a, b = _rows(rng, (4, 300)), _rows(rng, (4, 200))
    a[1] = 0
    b[2, 7] = np.nan
    a[3, 5] = np.inf
    y = rrm.model(a, b, True, dtype=np.float32)
    assert np.isfinite(y[0]).all() and not y[1].view(np.uint32).any() and np.isnan(y[2]).all() and np.isnan(y[3]).all()
    b[1, 0] = np.nan                                                        # a zero row and a NaN partner: NaN
    assert np.isnan(rrm.model(a, b, True, dtype=np.float32)[1]).all()


# ---- 2: the scaling rule, the very code of the kernel, under the sanitizers --------------------------------------
SANITIZED_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "smfft_rowconv_real_scale.hpp"
int main(int argc, char** argv) {
    for (int i = 1; i + 1 < argc; i += 2) {
        const unsigned mx = (unsigned)std::strtoul(argv[i], nullptr, 16), s = (unsigned)std::strtoul(argv[i + 1], nullptr, 16);
        const smfft::rowconv_real::RowScale r = smfft::rowconv_real::row_scale(mx, s);
        std::printf("%d %d %d %d\n", r.k, r.zero, r.finite, smfft::rowconv_real::max_exponent(mx));
    }
    return 0;
}
"""


def _f32_bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def test_scaling_rule_is_the_models_and_clean_under_asan_and_ubsan(tmp_path):
    """smfft_rowconv_real_scale.hpp alone, in a stand-alone host program with its own main, compiled with the host compiler and
    -fsanitize=address,undefined and run directly: exit 0, no report, and (k, zero, finite) equal to rowconv_real_model.exponent_rule
    over a table of (max, s): max in zero, the smallest subnormal, a large subnormal, FLT_MIN, 1, just under 2, 3, FLT_MAX, their
    negatives, Inf and NaN; s in 1, just under 2, 2, 3.99, 4, 7, 8, 100, 16383.5 and 4 * 4096 (odd and even exponents and the largest)"""
    gxx = shutil.which("g++") or shutil.which("clang++")
    if gxx is None:
        pytest.skip("no host C++ compiler")
    flt_max, flt_min, denorm = 3.4028234663852886e38, 1.1754943508222875e-38, 1.401298464324817e-45
    maxes = [0.0, denorm, 3 * denorm, flt_min * (1 - 2.0 ** -23), flt_min, 1.0, 2.0 - 2.0 ** -23, 3.0, 6.5e-20, 2.0 ** 100, flt_max, float("inf"), float("nan")]
    maxes += [-v for v in maxes[:-1]]
    sums = [1.0, 2.0 - 2.0 ** -23, 2.0, 3.99, 4.0, 7.0, 8.0, 100.0, 16383.5, 4.0 * 4096]
    table = [(mx, s) for mx in maxes for s in sums]
    src, exe = tmp_path / "rowconv_real_scale_main.cpp", tmp_path / "rowconv_real_scale_main"
    src.write_text(SANITIZED_MAIN)
    c = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-3000:]
    args = [f"{_f32_bits(v):08x}" for pair in table for v in pair]
    p = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr.strip(), p.stdout + p.stderr
    got = [tuple(int(w) for w in line.split()) for line in p.stdout.strip().split("\n")]
    assert len(got) == len(table)
    k, zero, finite = rrm.exponent_rule(np.array([t[0] for t in table], np.float32), np.array([t[1] for t in table], np.float32))
    for (mx, s), g, kk, z, f in zip(table, got, k, zero, finite):
        assert g[:3] == (int(kk), int(z), int(f)), (mx, s, g, int(kk), bool(z), bool(f))
    by = {(mx, s): g for (mx, s), g in zip(table, got) if mx == mx}
    assert by[(0.0, 1.0)][:3] == (0, 1, 1) and by[(float("inf"), 4.0)][:3] == (0, 0, 0) and got[len(sums) * 12][:3] == (0, 0, 0)      # zero, Inf, NaN
    assert by[(1.0, 1.0)] == (0, 0, 1, 0) and by[(1.0, 2.0)] == (0, 0, 1, 0) and by[(1.0, 4.0)] == (-1, 0, 1, 0) and by[(1.0, 16384.0)] == (-7, 0, 1, 0)
    assert by[(denorm, 1.0)] == (149, 0, 1, -149) and by[(flt_min, 1.0)] == (126, 0, 1, -126) and by[(flt_max, 16384.0)] == (-134, 0, 1, 127)
    assert by[(-3.0, 7.0)] == by[(3.0, 7.0)] == (-2, 0, 1, 1)
    header = open(os.path.join(CSRC, "smfft_rowconv_real_scale.hpp")).read()
    assert "#include" not in re.sub(r"//.*", "", header)                     # plain C++, integer arithmetic: no HIP header, no libm


# ---- 3: ISA budget and inventory -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """{M: assembly of smfft_rowconv_real_<M>.o as the Makefile compiles it}"""
    if not os.path.exists(ac.HIPCC):
        pytest.skip("hipcc not installed")
    return ac.addon_isa("smfft_rowconv_real", "ROWCONV_REAL", SIZES, tmp_path_factory.mktemp("rowconv_real_isa"))


def test_isa_budget_of_what_ships(isa):
    """per M exactly one kernel, read from the compiled object's metadata: no scratch, at most 256 VGPRs (two waves per SIMD), static LDS
    between 34,816 B (the transform region of 4096 points) and 256 B more (the reductions across waves at M = 2048 and 4096), no
    transcendentals, no packed f32 arithmetic; a thread's 32 row loads -- the kernel's only non-temporal loads, 4 bytes each -- go out up front with no branch
    or barrier between the first and the last; the sixteen stores are 4-byte, non-temporal and follow them"""
    total = 0
    for m, text in isa.items():
        descs = ac.descriptors(text)
        kernels = ac.pfb_kernels(text, "rowconv_real_kernel")
        assert len(descs) == 1 and set(descs) == set(kernels), (m, sorted(descs))
        total += len(descs)
        assert not re.search(r"\bscratch_", text), m
        (name, body), = kernels.items()
        assert "rowconv_real_kernelILi%dE" % m in name
        assert not [line for line in body if re.match(r"v_(sin|cos)_", line)], name
        assert not [line for line in body if re.match(r"v_pk_(add|mul|fma)_f32", line)], name
        assert ac.descriptor_field(descs, name, "private_segment_fixed_size") == 0, name
        v, lds = ac.descriptor_field(descs, name, "next_free_vgpr"), ac.descriptor_field(descs, name, "group_segment_fixed_size")
        print(f"M={m}: rowconv_real_kernel {v} VGPRs ({ac.occupancy(v)} waves per SIMD), {lds} B of LDS, 0 B of scratch")
        assert LDS_BUDGET <= lds <= LDS_BUDGET + LDS_REDUCTION and 2 * lds <= ac.LDS_PER_CU, (name, lds)
        assert v <= 256 and ac.occupancy(v) >= 2, (name, v)
        loads = [i for i, line in enumerate(body) if line.startswith("global_load") and re.search(r"\bnt\b", line)]      # (the others: twiddles)
        assert len(loads) == 32 and all(re.match(r"global_load_dword\s", body[i]) for i in loads), (name, len(loads))
        between = body[loads[0]:loads[-1] + 1]
        assert not [line for line in between if line.startswith(("s_cbranch", "s_branch", "s_setpc", "s_barrier"))], name
        stores = [i for i, line in enumerate(body) if line.startswith("global_store")]
        assert len(stores) == 16 and all(re.match(r"global_store_dword\s", body[i]) and re.search(r"\bnt\b", body[i]) for i in stores), (name, len(stores))
        assert min(stores) > max(loads), name
    assert total == 5


def test_library_ships_five_kernels_and_the_inventory_names_them(real_lib):
    ac.check_inventory(real_lib, rowconv_real_inventory.KERNELS, "smfft_rowconv_real_", 5, kinds=("tests", "bounds", "probes"))
    assert "permlane" in rowconv_real_inventory.__doc__ and "hostsim" in rowconv_real_inventory.__doc__


def test_isa_identity_compares_the_library():
    """tools/isa_identity.py compiles the five objects with the Makefile's flags and -I., like the other add-ons' (the tool itself
    needs the history of a git checkout and minutes of compiling: it is run by hand, DESIGN.md section 21 has its verdict)"""
    ac.check_isa_identity_lists("smfft_rowconv_real", "ROWCONV_REAL", SIZES)


# ---- 4: declarations and exports ---------------------------------------------------------------------------------
def test_python_mirror_matches_header(real_lib):
    from smfft_amd import rowconv, rowconv_real
    header = re.sub(r"[\s*]+", " ", open(os.path.join(ROOT, "include", "smfft_rowconv_real.h")).read())
    for phrase in ("Rows are float32. Row r of a is at element r n_a. Row r of b is at element r n_b. Row r of the output is at element r m. "
                   "All offsets are 64-bit. Let Lfull = n_a + n_b - 1.",
                   "This is np.convolve(a[r], b[r]).", "This is np.correlate(a[r], b[r], 'full'), so lag k - (n_b - 1) sits at index k.",
                   "np.convolve(a[r], b[r][::-1])", "out[r m + i] = y[r][first + i] for 0 <= i < m, with 0 <= first, 1 <= m and first + m <= Lfull",
                   "the same function as smfft_rowconv_fft_size", "scaling a[r] or b[r] by 2^s scales row r of the result by 2^s to the bit",
                   "as long as nothing leaves the normal fp32 range", "Out of scope", "complex rows (that is smfft_rowconv_ )",
                   "two row pairs in one transform slot", "results or intermediate sums outside the normal fp32 range",
                   "Lfull > 4096 (that is the large engine's ground)", "one b shared by all rows (that is smfft_fir_real_ )",
                   "a peak / arg-max output over the lags", "shrinking M for narrow windows", "strided rows",
                   "d_a == d_b is allowed", "every output element is written exactly once", "4-byte alignment",
                   "only a[0, batch n_a), b[0, batch n_b) and out[0, batch m) are touched",
                   "the bits of row r's outputs depend only on a[r], b[r], n_a, n_b and the mode",
                   "A NaN or Inf anywhere in a pair makes all outputs of that pair NaN and touches no other row",
                   "A pair with an all-zero row and a finite partner stores +0 in every element",
                   "batch == 0 launches nothing and returns 0"):
        assert phrase in header, phrase
    decl = ac.declarations("smfft_rowconv_real.h")
    assert sorted(decl) == sorted(rowconv_real.SIGS) == sorted(NAMES)
    for name, (res, args) in decl.items():
        assert rowconv_real.SIGS[name] == ac.signature(res, args), name
        assert rowconv_real.SIGS[name] == rowconv.SIGS[name.replace("_real", "")], name      # the argument lists of smfft_rowconv_*
    assert rowconv_real.SIZES == SIZES and rowconv_real.MAX_FULL == 4096


def test_library_exports_exactly_the_four_symbols(real_lib):
    ac.check_exports(real_lib, NAMES)


# ---- 5: rejections -------------------------------------------------------------------------------------------------
def test_unsupported_combinations_return_minus_one_without_a_device(real_lib):
    """-1 (or 0 for an empty batch) before any HIP call: run in a process where no GPU is visible, with addresses that are never read.
    d_out == d_a and d_out == d_b are refused whatever the batch; d_a == d_b is not"""
    code = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
ll, d, vp, i = ctypes.c_longlong, ctypes.c_double, ctypes.c_void_p, ctypes.c_int
head = [vp, vp, vp, i, i, i, i, ll, i]
lib.smfft_rowconv_real_launch.argtypes = head + [vp]
lib.smfft_rowconv_real_launch_tuned.argtypes = head + [vp, i]
lib.smfft_rowconv_real_benchmark.argtypes = head + [ctypes.POINTER(d)]
t = d(0.0)
A, B, OUT = 4096, 8192, 16384
def calls(n_a, n_b, first, m, batch, grid=3, da=A, db=B, dout=OUT):
    out = []
    for c in (0, 1, 7):
        out += [lib.smfft_rowconv_real_launch(da, db, dout, n_a, n_b, first, m, batch, c, None),
                lib.smfft_rowconv_real_launch_tuned(da, db, dout, n_a, n_b, first, m, batch, c, None, grid),
                lib.smfft_rowconv_real_benchmark(da, db, dout, n_a, n_b, first, m, batch, c, ctypes.byref(t))]
    return out
rc = []
# sizes outside the range
for n_a, n_b in ((0, 5), (5, 0), (-5, 5), (5, -5), (4097, 1), (1, 4097), (2049, 2049), (4096, 2), (2**31 - 1, 2**31 - 1), (2**31 - 1, 3)):
    rc += calls(n_a, n_b, 0, 1, 10) + calls(n_a, n_b, 0, 1, 0) + [lib.smfft_rowconv_real_fft_size(n_a, n_b)]
# windows outside the full result of (300, 200): Lfull = 499
for first, m in ((-1, 5), (0, 0), (0, -3), (0, 500), (1, 499), (499, 1), (498, 2), (2**31 - 1, 1), (1, 2**31 - 1), (2**31 - 1, 2**31 - 1)):
    rc += calls(300, 200, first, m, 10) + calls(300, 200, first, m, 0)
# batch < 0; grid < 1, for an empty batch too
for n_a, n_b in ((1, 1), (300, 200), (2048, 2049), (4096, 1)):
    rc += calls(n_a, n_b, 0, 1, -1)
    for grid in (0, -1):
        rc += [lib.smfft_rowconv_real_launch_tuned(A, B, OUT, n_a, n_b, 0, 1, batch, 0, None, grid) for batch in (10, 0)]
# the output is an input: refused, for an empty batch and for null == null too
for n_a, n_b in ((300, 200), (1, 1), (2048, 2048)):
    for batch in (10, 0):
        rc += calls(n_a, n_b, 0, 1, batch, dout=A) + calls(n_a, n_b, 0, 1, batch, dout=B) + calls(n_a, n_b, 0, 1, batch, da=A, db=A, dout=A)
        rc += calls(n_a, n_b, 0, 1, batch, da=None, db=None, dout=None) + calls(n_a, n_b, 0, 1, batch, da=None, dout=None) + calls(n_a, n_b, 0, 1, batch, db=None, dout=None)
empty = []
for n_a, n_b, first, m in ((1, 1, 0, 1), (300, 200, 0, 499), (300, 200, 498, 1), (2048, 2049, 2045, 7), (4096, 1, 0, 4096), (1, 4096, 4095, 1)):
    empty += calls(n_a, n_b, first, m, 0) + calls(n_a, n_b, first, m, 0, da=A, db=A)             # d_a == d_b is allowed
sizes = [lib.smfft_rowconv_real_fft_size(*s) for s in ((1, 1), (128, 129), (129, 129), (300, 200), (1000, 25), (1000, 26), (4096, 1), (2048, 2049))]
print(rc, empty, t.value, sizes)
sys.exit(0 if rc and rc == [-1] * len(rc) and empty == [0] * 108 and t.value == 0.0 and sizes == [256, 256, 512, 512, 1024, 2048, 4096, 4096] else 1)
"""
    p = subprocess.run([sys.executable, "-c", code, real_lib], capture_output=True, text=True, timeout=120, env=dict(os.environ, **NO_DEVICE))
    assert p.returncode == 0, p.stdout + p.stderr


def test_python_wrappers_refuse_before_a_device(real_lib):
    from smfft_amd import rowconv_real
    A, B, OUT = 4096, 8192, 16384
    for n_a, n_b in ((0, 5), (5, 0), (-5, 5), (4097, 1), (1, 4097), (2049, 2049)):
        with pytest.raises(RuntimeError):
            rowconv_real.launch(A, B, OUT, n_a, n_b, 0, 1, 10)
        with pytest.raises(RuntimeError):
            rowconv_real.launch_tuned(A, B, OUT, n_a, n_b, 0, 1, 10, 3)
        assert rowconv_real.benchmark(A, B, OUT, n_a, n_b, 0, 1, 10) == (-1, 0.0)
        with pytest.raises(ValueError):
            rowconv_real.fft_size(n_a, n_b)
    for first, m in ((-1, 5), (0, 0), (0, 500), (499, 1), (498, 2)):
        with pytest.raises(RuntimeError):
            rowconv_real.launch(A, B, OUT, 300, 200, first, m, 10, correlate=True)
        with pytest.raises(ValueError):
            rowconv_real.convolve(np.zeros(300), np.zeros(200), first=first, m=m)
    with pytest.raises(RuntimeError):
        rowconv_real.launch(A, B, OUT, 300, 200, 0, 499, -1)
    for dout in (A, B):
        for batch in (10, 0):                                        # the output is an input: refused for an empty batch too
            with pytest.raises(RuntimeError):
                rowconv_real.launch(A, B, dout, 300, 200, 0, 499, batch)
            with pytest.raises(RuntimeError):
                rowconv_real.launch_tuned(A, B, dout, 300, 200, 0, 499, batch, 3)
            assert rowconv_real.benchmark(A, B, dout, 300, 200, 0, 499, batch) == (-1, 0.0)
    for grid in (0, -1):
        with pytest.raises(RuntimeError):
            rowconv_real.launch_tuned(A, B, OUT, 300, 200, 0, 499, 10, grid)
    rowconv_real.launch(A, A, OUT, 300, 300, 0, 599, 0, correlate=True)   # d_a == d_b, an empty batch: nothing is launched
    assert rowconv_real.benchmark(A, B, OUT, 300, 200, 0, 499, 0) == (0, 0.0)
    for a, b in ((np.zeros(5, np.complex64), np.zeros(3)), (np.zeros(5), np.zeros(3, np.complex128)), (np.zeros((2, 5), np.complex64), np.zeros((2, 3), np.complex64))):
        with pytest.raises(TypeError, match="smfft_amd.rowconv"):
            rowconv_real.convolve(a, b)
    with pytest.raises(ValueError):
        rowconv_real.convolve(np.zeros(4096, np.float32), np.zeros(2, np.float32))
    with pytest.raises(ValueError):
        rowconv_real.convolve(np.zeros((3, 0), np.float32), np.zeros((3, 5), np.float32))
    with pytest.raises(ValueError):
        rowconv_real.convolve(np.zeros((3, 5), np.float32), np.zeros((2, 5), np.float32))     # rows do not pair
    with pytest.raises(ValueError):
        rowconv_real.convolve(np.float32(1), np.zeros(5, np.float32))
    assert rowconv_real.fft_size(300, 200) == 512


def test_import_does_not_load_the_library():
    ac.check_import_does_not_load("rowconv_real", "smfft_rowconv_real")

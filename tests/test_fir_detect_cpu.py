"""CPU checks of the detected outputs of the overlap-save FIR filter banks (smfft_amd/csrc/smfft_fir_detect.hip,
libsmfft_fir_detect.so): the fp64 model (tools/fir_detect_model.py) is |np.convolve|^2 / |np.correlate|^2 and its running best filter
is np.max / np.argmax, NaN included; the gfx950 code of every kernel keeps the budgets of DESIGN.md section 17 and the occupancy of the
complex bank's kernel; and the C ABI declares, exports and validates the four entry points without a device.  No GPU code is run
(hipcc cross-compiles gfx950)."""
import concurrent.futures
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fir_detect_model as fdm  # noqa: E402

from tests import addon_checks as ac  # noqa: E402
from tests import fir_detect_inventory  # noqa: E402

HIPCC = ac.HIPCC
CSRC = ac.CSRC
LIB = os.path.join(ROOT, "smfft_amd", "libsmfft_fir_detect.so")
SIZES = (256, 512, 1024, 2048, 4096)
NAMES = ("smfft_fir_power_launch", "smfft_fir_power_benchmark", "smfft_fir_peak_launch", "smfft_fir_peak_benchmark")
LDS_BYTES = 4096 // 16 * 17 * 8
WINNERS_LDS = (0, 16 * 256 * 4, 2 * 16 * 256 * 4)       # nothing, the indices, or the powers and the indices of 256 threads x 16 elements
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def detect_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", CSRC, "-j", "4", "../libsmfft_fir_detect.so"])
    return LIB


# ---- the model ---------------------------------------------------------------------------------------
def _crand(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("correlate", [False, True])
def test_model_is_numpys_power_and_argmax(n, correlate):
    """the plan's segmentation in fp64: the power is |np.convolve|^2 / |np.correlate|^2 and the running best filter is np.max /
    np.argmax along the filters"""
    rng = np.random.default_rng(n + correlate)
    worst = 0.0
    for m in ac.fir_taps_cases(n):
        for length in ac.fir_length_cases(n, m):
            if length < 1:
                continue
            x, h = _crand(rng, (2, length)), _crand(rng, (3, m))
            want = fdm.direct_power(x, h, correlate)
            got = fdm.power(x, h, n, correlate)
            err = np.max(np.abs(got - want)) / np.max(want)
            worst = max(worst, err)
            assert err <= 1e-12, (n, m, length, correlate, err)
            best, index = fdm.peak(x, h, n, correlate)
            assert index.dtype == np.int32 and best.shape == index.shape == (2, length)
            assert np.array_equal(best, np.max(got, axis=1)) and np.array_equal(index, np.argmax(got, axis=1)), (n, m, length, correlate)
    print(f"N={n} correlate={correlate}: max |model - numpy| / max |numpy| = {worst:.2e}")


def test_running_best_is_numpys_rule_with_ties_and_nans():
    """ties go to the lowest filter, a NaN beats every number (an infinity too) and the first NaN wins: np.max / np.argmax"""
    nan, inf = np.nan, np.inf
    columns = [[1, 1, 1], [0, 0, 0], [1, 2, 2], [2, 1, 2], [nan, 1, 2], [1, nan, 2], [1, 2, nan], [nan, nan, 1], [1, nan, nan],
               [inf, nan, inf], [inf, inf, 1], [0, inf, nan], [3, 2, 1]]
    p = np.array(columns, np.float64).T[None]                      # (1, K = 3, L)
    best, index = fdm.running_peak(p)
    assert np.array_equal(index[0], np.argmax(p[0], axis=0))
    assert np.array_equal(best[0], np.max(p[0], axis=0), equal_nan=True)
    assert list(index[0]) == [0, 0, 1, 0, 0, 1, 2, 0, 1, 1, 0, 2, 0]
    rng = np.random.default_rng(3)
    q = rng.integers(0, 4, (2, 7, 500)).astype(np.float32)           # many ties
    q[rng.random(q.shape) < 0.05] = np.nan
    best, index = fdm.running_peak(q)
    assert np.array_equal(index, np.argmax(q, axis=1)) and np.array_equal(best, np.max(q, axis=1), equal_nan=True)


# ---- ISA ---------------------------------------------------------------------------------------------------
def _bodies(text, frag):
    found = {}
    for m in re.finditer(r"^(_Z\w*%s\w*):[^\n]*\n(.*?)\n\s*s_endpgm" % frag, text, re.S | re.M):
        found[m.group(1)] = [line.strip() for line in m.group(2).split("\n")]
    return found


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """{N: assembly of smfft_fir_detect_<N>.o as the Makefile compiles it}, and the assembly of the main library's smfft_fir.hip"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    tmp = tmp_path_factory.mktemp("fir_detect_isa")

    def compile_one(n):
        if n == 0:
            return ac.device_asm(os.path.join(CSRC, "smfft_fir.hip"), [], tmp / "smfft_fir.s")
        return ac.device_asm(os.path.join(CSRC, "smfft_fir_detect.hip"), ["-I" + CSRC] + ac.makefile_flags("FIR_DETECT", n) + [f"-DSMFFT_FIR_DETECT_N={n}"],
                             tmp / f"smfft_fir_detect_{n}.s")
    with concurrent.futures.ThreadPoolExecutor(6) as pool:
        texts = list(pool.map(compile_one, SIZES + (0,)))
    return dict(zip(SIZES, texts[:-1])), texts[-1]


def _loop_depths(body):
    """per line of a kernel body, the loop depth of its basic block, from the annotations the compiler writes behind a block's label
    ("in Loop: Header=BB0_6 Depth=1", "This Inner Loop Header: Depth=2"); a block without one lies in no loop.  Blocks that the
    compiler moves out of line keep their annotation, so this does not depend on where a block is laid out."""
    depths, depth, i = [], 0, 0
    while i < len(body):
        if re.match(r"(\.LBB\d+_\d+:|; %bb\.\d+:)", body[i]):
            notes, j = body[i], i + 1
            while j < len(body) and body[j].startswith(";") and not body[j].startswith("; %bb."):
                notes, j = notes + body[j], j + 1
            depth = max([int(d) for d in re.findall(r"Depth=(\d+)", notes)], default=0)
        depths.append(depth)
        i += 1
    return depths


def test_isa_budget_of_what_ships(isa):
    """per length exactly two kernels: no scratch, the LDS of 4096 points (the peak kernel: plus its winners where they live there, two
    workgroups still fitting a compute unit), no transcendentals, no packed f32 arithmetic; the 16 signal loads of a segment -- the
    kernels' only non-temporal loads -- go out with no branch, barrier or vmcnt(0) wait between the first and the last, inside the tile
    loop and in front of the filter loop; the power kernel's stores are 16 dword stores inside the filter loop, the peak kernel's 32
    dword stores lie behind it; the registers are those DESIGN.md section 17 states and allow the occupancy of the complex bank's
    fir_overlap_save_kernel<N>, two waves per SIMD, compiled here from smfft_fir.hip with the main library's flags"""
    detect, cplx = isa
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    cdescs = ac.descriptors(cplx)
    total = 0
    for n, text in detect.items():
        descs = ac.descriptors(text)
        power, peak = _bodies(text, "fir_power_kernel"), _bodies(text, "fir_peak_kernel")
        assert len(descs) == 2 and len(power) == 1 and len(peak) == 1 and set(descs) == set(power) | set(peak), (n, sorted(descs))
        total += len(descs)
        assert not re.search(r"\bscratch_", text), n
        cname = next(k for k in cdescs if "fir_overlap_save_kernelILi%dE" % n in k)
        vc = ac.descriptor_field(cdescs, cname, "next_free_vgpr")
        assert ac.occupancy(vc) == 2, (n, vc)
        for kind, (name, body) in (("power", next(iter(power.items()))), ("peak", next(iter(peak.items())))):
            assert "ILi%dE" % n in name
            assert not [line for line in body if line.startswith("scratch_")], name
            assert not [line for line in body if re.match(r"v_(sin|cos)_", line)], name
            assert not [line for line in body if re.match(r"v_pk_(add|mul|fma)_f32", line)], name
            assert ac.descriptor_field(descs, name, "private_segment_fixed_size") == 0, name
            lds = ac.descriptor_field(descs, name, "group_segment_fixed_size")
            assert lds - LDS_BYTES in (WINNERS_LDS if kind == "peak" else (0,)) and 2 * lds <= LDS_PER_CU, (name, lds)
            # the signal loads
            loads = [i for i, line in enumerate(body) if line.startswith("global_load") and re.search(r"\bnt\b", line)]
            assert len(loads) == 16 and all(re.match(r"global_load_dwordx2\s", body[i]) for i in loads), (name, len(loads))
            between = body[loads[0]:loads[-1] + 1]
            assert not [line for line in between if line.startswith(("s_cbranch", "s_branch", "s_setpc", "s_barrier"))], name
            assert not [line for line in between if re.search(r"vmcnt\(0\)", line)], name
            # the loops: the signal loads in the tile loop (depth 1), in front of the filter loop (depth 2)
            depth = _loop_depths(body)
            assert max(depth) == 2 and {depth[i] for i in loads} == {1}, name
            stores = [i for i, line in enumerate(body) if line.startswith("global_store")]
            assert all(re.match(r"global_store_dword\s", body[i]) for i in stores), name
            if kind == "power":
                assert len(stores) == 16 and {depth[i] for i in stores} == {2}, (name, len(stores))      # 16 per filter, in the filter loop
            else:
                assert len(stores) == 32 and {depth[i] for i in stores} == {1}, (name, len(stores))      # once per segment, behind the filter loop
            v = ac.descriptor_field(descs, name, "next_free_vgpr")
            print(f"N={n}: fir_{kind}_kernel {v} VGPRs (complex bank: {vc}), {lds} B of LDS")
            assert v <= 256 and ac.occupancy(v) >= ac.occupancy(vc), (name, v, vc)
            assert f"`fir_{kind}_kernel<{n}>` | {v} | {lds} |" in design, f"DESIGN.md section 17 states other figures than {v} VGPRs / {lds} B for fir_{kind}_kernel<{n}>"
    assert total == 10


def test_library_ships_ten_kernels_and_the_inventory_names_them(detect_lib):
    ac.check_inventory(detect_lib, fir_detect_inventory.KERNELS, "smfft_fir_", 10, kinds=("tests", "bounds", "probes"))
    assert "permlane" in fir_detect_inventory.__doc__ and "hostsim" in fir_detect_inventory.__doc__


# ---- C ABI and Python mirror ---------------------------------------------------------------------------------
def test_python_mirror_matches_header(detect_lib):
    from smfft_amd import fir_detect
    header = re.sub(r"[\s*]+", " ", open(os.path.join(ROOT, "include", "smfft_fir_detect.h")).read())
    for phrase in ("Out of scope", "real signals", "N >= 8192", "thresholded candidate lists", "a maximum over samples rather than filters",
                   "There is no prepare function", "smfft_fir_prepare", "ONE filter group", "fills fewer workgroups", "first NaN wins"):
        assert phrase in header, phrase
    decl = ac.declarations("smfft_fir_detect.h")
    assert sorted(decl) == sorted(fir_detect.SIGS) == sorted(NAMES)
    for name, (res, args) in decl.items():
        assert res == "int" and fir_detect.SIGS[name] == ac.signature(res, args), name
    assert fir_detect.SIZES == SIZES
    # the argument lists are those of smfft_fir_launch / smfft_fir_benchmark of include/smfft.h with the output changed
    base = ac.declarations("smfft.h")

    def words(args):
        return [re.sub(r"\s+", " ", a.strip()) for a in args.split(",")]
    for form in ("launch", "benchmark"):
        ref = words(base["smfft_fir_" + form][1])
        assert ref[8] == "void* d_output"
        assert words(decl["smfft_fir_power_" + form][1]) == ref[:8] + ["void* d_power"] + ref[9:]
        assert words(decl["smfft_fir_peak_" + form][1]) == ref[:8] + ["void* d_peak", "void* d_index"] + ref[9:]


def test_library_exports_exactly_the_four_symbols(detect_lib):
    nm = subprocess.run(["nm", "-D", "--defined-only", detect_lib], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r" T (smfft_\w+)$", nm, re.M)) == sorted(NAMES)


def test_unsupported_combinations_return_minus_one_without_a_device(detect_lib):
    """-1 (or 0 for an empty signal) before any HIP call: run in a process where no GPU is visible, with null pointers, over the four
    functions; the cases are those of tests/addon_checks.py check_fir_rejections"""
    code = r"""
import ctypes, sys
lib, sizes = ctypes.CDLL(sys.argv[1]), [int(a) for a in sys.argv[2:]]
ll = ctypes.c_longlong
t = ctypes.c_double(0.0)
def calls(L, C, K, M, N, corr):
    return [lib.smfft_fir_power_launch(None, ll(L), C, None, K, M, N, corr, None, None),
            lib.smfft_fir_power_benchmark(None, ll(L), C, None, K, M, N, corr, None, ctypes.byref(t)),
            lib.smfft_fir_peak_launch(None, ll(L), C, None, K, M, N, corr, None, None, None),
            lib.smfft_fir_peak_benchmark(None, ll(L), C, None, K, M, N, corr, None, None, ctypes.byref(t))]
lo, hi = sizes[0], sizes[-1]
off = [lo // 2, 2 * hi, lo - 1, 1000, 0, -lo]
bad = [(1000, 1, 1, 17, n) for n in off]                                                   # (L, C, K, M, N)
bad += [(1000, 1, 1, m, n) for n in sizes for m in (0, n, -3)]
bad += [(1000, 1, k, 17, n) for n in (lo, hi) for k in (0, -2)] + [(1000, c, 1, 17, n) for n in (lo, hi) for c in (0, -1)]
bad += [(L, 1, 1, 17, n) for n in (lo, hi) for L in (-1, -5)]
rc = []
for L, C, K, M, N in bad:
    for corr in (0, 1):
        rc += calls(L, C, K, M, N, corr)
empty = []
for n in sizes:
    for corr in (0, 1):
        empty += calls(0, 1, 1, 17, n, corr)
print(rc, empty, t.value)
sys.exit(0 if rc == [-1] * len(rc) and len(rc) == 8 * len(bad) and empty == [0] * (8 * len(sizes)) and t.value == 0.0 else 1)
"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code, detect_lib] + [str(n) for n in SIZES], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stdout + p.stderr


def test_python_wrappers_refuse_before_a_device(detect_lib):
    from smfft_amd import fir_detect
    for n in (SIZES[0], SIZES[-1]):
        with pytest.raises(RuntimeError):
            fir_detect.power_launch(None, 1000, 1, None, 1, n, n, None)
        with pytest.raises(RuntimeError):
            fir_detect.peak_launch(None, 1000, 1, None, 1, n, n, None, None)
        with pytest.raises(ValueError):
            fir_detect.power_launch(None, 1000, 1, None, 1, 17, n, None, mode="xcorr")
        with pytest.raises(ValueError):
            fir_detect.peak_launch(None, 1000, 1, None, 1, 17, n, None, None, mode="xcorr")
    assert fir_detect.power_benchmark(None, 1000, 1, None, 1, 17, 8192, None) == (-1, 0.0)
    assert fir_detect.peak_benchmark(None, 1000, 1, None, 1, 17, 8192, None, None) == (-1, 0.0)
    with pytest.raises(ValueError):
        fir_detect.peak_benchmark(None, 1000, 1, None, 1, 17, 1024, None, None, mode="both")
    x, h = np.zeros(10, np.complex64), np.zeros(17, np.complex64)
    for fn in (fir_detect.power, fir_detect.peak):
        with pytest.raises(ValueError):
            fn(x, h, mode="xcorr")
        with pytest.raises(ValueError):
            fn(np.zeros((2, 2, 10), np.complex64), h)
        with pytest.raises(ValueError):
            fn(x, np.zeros((2, 2, 17), np.complex64))
        with pytest.raises(ValueError):
            fn(x, np.zeros(4096, np.complex64))                  # the 4 M rule's range: 1 ... 4095 taps
        with pytest.raises(ValueError):
            fn(x, h, fft_size=8192)
        with pytest.raises(ValueError):
            fn(x, np.zeros(256, np.complex64), fft_size=256)


def test_import_does_not_load_the_library():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import smfft_amd, smfft_amd.fir_detect as l; assert l._lib is None; "
            "maps = open('/proc/self/maps').read(); assert 'libsmfft_fir_detect' not in maps; print('ok')")
    p = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout + p.stderr

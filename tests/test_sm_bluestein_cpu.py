"""CPU checks of the arbitrary-length FFTs (smfft_amd/csrc/smfft_bluestein.hip, libsmfft_bluestein.so): the fp64 model
(tools/bluestein_model.py) is np.fft.fft / np.fft.ifft * n; the library's host-built tables are the model's, rounded once to fp32; the
table builder runs clean under the address and undefined-behaviour sanitizers as a stand-alone host program; the gfx950 code of the
five kernels keeps the FIR bank's budget; and the C ABI declares, exports and validates the seven entry points without a device.  No GPU
code is run (hipcc cross-compiles gfx950)."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bluestein_model as bm  # noqa: E402

from tests import addon_checks as ac  # noqa: E402
from tests import bluestein_inventory  # noqa: E402

CSRC = ac.CSRC
LIB = os.path.join(ROOT, "smfft_amd", "libsmfft_bluestein.so")
SIZES = (256, 512, 1024, 2048, 4096)
LENGTHS = (1, 2, 3, 127, 128, 129, 1000, 1021, 2047, 2048)
NAMES = ("smfft_bluestein_fft_size", "smfft_bluestein_plan_bytes", "smfft_bluestein_tables", "smfft_bluestein_prepare",
         "smfft_bluestein_launch", "smfft_bluestein_launch_tuned", "smfft_bluestein_benchmark")
LDS_BYTES = 4096 // 16 * 17 * 8


@pytest.fixture(scope="module")
def bluestein_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", CSRC, "-j", "4", "../libsmfft_bluestein.so"])
    return LIB


# ---- 1: the model -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [False, True])
def test_model_is_numpys_fft(inverse):
    """the chain pad, FFT_M, product with B M, IFFT_M, window with the plan's fp64 tables equals np.fft.fft / np.fft.ifft * n within
    1e-12 of the largest output"""
    rng = np.random.default_rng(int(inverse))
    for n in LENGTHS:
        x = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
        want = np.fft.ifft(x, axis=-1) * n if inverse else np.fft.fft(x, axis=-1)
        err = np.max(np.abs(bm.model(x, n, inverse) - want)) / np.max(np.abs(want))
        print(f"n={n} inverse={inverse}: max |model - numpy| / max |numpy| = {err:.2e}")
        assert err <= 1e-12, (n, inverse, err)


def test_fft_size_is_minimal_and_flips_at_the_boundaries():
    sizes = [bm.fft_size(n) for n in range(1, 2049)]
    for n, m in zip(range(1, 2049), sizes):
        assert m in SIZES and m >= 2 * n - 1 and (m == 256 or m // 2 < 2 * n - 1), (n, m)
    assert [n for n in range(2, 2049) if sizes[n - 1] != sizes[n - 2]] == [129, 257, 513, 1025]
    assert sizes[0] == sizes[127] == 256 and sizes[2047] == 4096
    for n in (0, -1, 2049):
        with pytest.raises(ValueError):
            bm.fft_size(n)
    for m, (lo, hi) in bluestein_inventory.LENGTHS.items():
        assert bm.fft_size(lo) == bm.fft_size(hi) == m and (lo == 1 or bm.fft_size(lo - 1) == m // 2)


# ---- 2: the tables -------------------------------------------------------------------------------------------
def test_tables_are_the_models_rounded_once(bluestein_lib, tmp_path):
    """smfft_bluestein_tables in a process with no visible device: every component within half an fp32 ulp (+ 1e-12 of fp64 slack) of the
    model's fp64 value -- a table built in fp32, or from float(j * j), fails --, W zero from n on, B symmetric to the bit"""
    code = r"""
import ctypes, sys
import numpy as np
lib = ctypes.CDLL(sys.argv[1])
lib.smfft_bluestein_plan_bytes.restype = ctypes.c_longlong
lib.smfft_bluestein_tables.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
out = {}
for n in [int(a) for a in sys.argv[3:]]:
    for inverse in (0, 1):
        m = lib.smfft_bluestein_fft_size(n)
        assert lib.smfft_bluestein_plan_bytes(n) == 16 * m
        guarded = np.full(2 * m + 64, np.complex64(7 - 7j))
        assert lib.smfft_bluestein_tables(n, inverse, guarded.ctypes.data + 8 * 32) == 0
        assert np.all(guarded[:32] == 7 - 7j) and np.all(guarded[-32:] == 7 - 7j)
        out[f"{n}_{inverse}"] = guarded[32:-32].copy()
np.savez(sys.argv[2], **out)
"""
    path = str(tmp_path / "tables.npz")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code, bluestein_lib, path] + [str(n) for n in LENGTHS], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    got_all = np.load(path)
    for n in LENGTHS:
        m = bm.fft_size(n)
        for inverse in (0, 1):
            got, want = got_all[f"{n}_{inverse}"], bm.plan(n, bool(inverse))
            assert got.dtype == np.complex64 and got.shape == want.shape == (2 * m,)
            for g, w in ((got.real, want.real), (got.imag, want.imag)):
                excess = np.abs(g.astype(np.float64) - w) - (2.0 ** -24 * np.abs(w) + 1e-12)
                assert np.all(excess <= 0), (n, inverse, int(np.argmax(excess)), float(np.max(excess)))
            assert not got[n:m].any(), (n, inverse)
            B = got[m:]
            assert np.array_equal(np.ascontiguousarray(B[1:]).view(np.uint64), np.ascontiguousarray(B[:0:-1]).view(np.uint64)), (n, inverse)


def test_mirror_tables_and_sizes(bluestein_lib):
    from smfft_amd import bluestein
    for n in (1, 129, 1000, 2048):
        m = bm.fft_size(n)
        assert bluestein.fft_size(n) == m and bluestein.plan_bytes(n) == 16 * m
        t = bluestein.tables(n, inverse=True)
        assert t.dtype == np.complex64 and t.shape == (2 * m,)
        assert np.array_equal(t[:n], np.conj(bluestein.tables(n)[:n]))


# ---- 3: the table builder under the sanitizers ---------------------------------------------------------------
SANITIZED_MAIN = r"""
#include <cstdio>
#include <vector>
#include "smfft_bluestein_tables.hpp"
int main() {
    const int lengths[] = {1, 2, 3, 127, 128, 129, 1000, 1021, 2047, 2048};
    double sum = 0.0;
    for (int n : lengths) {
        for (int inverse = 0; inverse < 2; ++inverse) {
            const int M = smfft::bluestein::fft_size(n);
            std::vector<float> plan(4 * (size_t)M);          // exactly the plan: a write past it is a heap overflow
            smfft::bluestein::build_tables(n, inverse != 0, plan.data());
            for (float v : plan) sum += v;
        }
    }
    if (smfft::bluestein::fft_size(0) != -1 || smfft::bluestein::fft_size(2049) != -1) return 2;
    std::printf("%.6f\n", sum);
    return 0;
}
"""


def test_table_builder_is_clean_under_asan_and_ubsan(tmp_path):
    """the plain C++ header alone, in a stand-alone host program with its own main, compiled with g++ -fsanitize=address,undefined:
    exit 0 and no report.  Host code only: nothing of it is loaded into python and no device is involved"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not installed")
    src, exe = tmp_path / "bluestein_tables_main.cpp", tmp_path / "bluestein_tables_main"
    src.write_text(SANITIZED_MAIN)
    c = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr.strip(), p.stdout + p.stderr
    assert re.fullmatch(r"-?\d+\.\d+\n", p.stdout), p.stdout
    header = open(os.path.join(CSRC, "smfft_bluestein_tables.hpp")).read()
    assert "hip" not in re.sub(r"//.*", "", header).lower()      # plain C++: no HIP in the code


# ---- 4: ISA budget and inventory -------------------------------------------------------------------------------
def _loop_depths(body):
    """per line of a kernel body, the loop depth of its basic block, from the annotations the compiler writes behind a block's label
    ("in Loop: Header=BB0_6 Depth=1", "This Inner Loop Header: Depth=2"); a block without one lies in no loop"""
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


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """{M: assembly of smfft_bluestein_<M>.o as the Makefile compiles it}"""
    if not os.path.exists(ac.HIPCC):
        pytest.skip("hipcc not installed")
    return ac.addon_isa("smfft_bluestein", "BLUESTEIN", SIZES, tmp_path_factory.mktemp("bluestein_isa"))


def test_isa_budget_of_what_ships(isa):
    """per M exactly one kernel: no scratch, at most 256 VGPRs (two waves per SIMD, the FIR bank's occupancy), the LDS of 4096 points,
    no transcendentals, no packed f32 arithmetic; a thread's eight row loads -- the kernel's only non-temporal loads -- go out with no
    branch, barrier or vmcnt(0) wait between the first and the last, inside the tile loop; its eight stores are there too; the loads of
    the two tables lie in front of the loop"""
    total = 0
    for m, text in isa.items():
        descs = ac.descriptors(text)
        kernels = ac.pfb_kernels(text, "bluestein_kernel")
        assert len(descs) == 1 and set(descs) == set(kernels), (m, sorted(descs))
        total += len(descs)
        assert not re.search(r"\bscratch_", text), m
        (name, body), = kernels.items()
        assert "bluestein_kernelILi%dE" % m in name
        assert not [line for line in body if re.match(r"v_(sin|cos)_", line)], name
        assert not [line for line in body if re.match(r"v_pk_(add|mul|fma)_f32", line)], name
        assert ac.descriptor_field(descs, name, "private_segment_fixed_size") == 0, name
        v, lds = ac.descriptor_field(descs, name, "next_free_vgpr"), ac.descriptor_field(descs, name, "group_segment_fixed_size")
        print(f"M={m}: bluestein_kernel {v} VGPRs ({ac.occupancy(v)} waves per SIMD), {lds} B of LDS")
        assert lds == LDS_BYTES, (name, lds)
        assert v <= 256 and ac.occupancy(v) >= 2, (name, v)
        loads = [i for i, line in enumerate(body) if line.startswith("global_load") and re.search(r"\bnt\b", line)]
        assert len(loads) == 8 and all(re.match(r"global_load_dwordx2\s", body[i]) for i in loads), (name, len(loads))
        between = body[loads[0]:loads[-1] + 1]
        assert not [line for line in between if line.startswith(("s_cbranch", "s_branch", "s_setpc", "s_barrier"))], name
        assert not [line for line in between if re.search(r"vmcnt\(0\)", line)], name
        stores = [i for i, line in enumerate(body) if line.startswith("global_store")]
        assert len(stores) == 8 and all(re.match(r"global_store_dwordx2\s", body[i]) and re.search(r"\bnt\b", body[i]) for i in stores), (name, len(stores))
        # the loops: the row loads and the stores in the tile loop (depth 1, the only loop), every other load -- the two tables and the
        # engines' twiddles -- in front of it
        depth = _loop_depths(body)
        assert max(depth) == 1 and {depth[i] for i in loads} == {1} and {depth[i] for i in stores} == {1}, name
        tables = [i for i, line in enumerate(body) if line.startswith("global_load") and not re.search(r"\bnt\b", line)]
        assert len(tables) >= 24 and {depth[i] for i in tables} == {0} and max(tables) < loads[0], (name, len(tables))
    assert total == 5


def test_library_ships_five_kernels_and_the_inventory_names_them(bluestein_lib):
    ac.check_inventory(bluestein_lib, bluestein_inventory.KERNELS, "smfft_bluestein_", 5, kinds=("tests", "bounds", "probes"))
    assert "permlane" in bluestein_inventory.__doc__ and "hostsim" in bluestein_inventory.__doc__


# ---- 5: declarations and exports ---------------------------------------------------------------------------------
def test_python_mirror_matches_header(bluestein_lib):
    from smfft_amd import bluestein
    header = re.sub(r"[\s*]+", " ", open(os.path.join(ROOT, "include", "smfft_bluestein.h")).read())
    for phrase in ("Out of scope", "n > 2048", "real input", "strided or transposed rows", "chirp-z", "smfft_launch computes them more cheaply",
                   "d_out == d_in", "rounded once to fp32", "UN-normalised"):
        assert phrase in header, phrase
    decl = ac.declarations("smfft_bluestein.h")
    assert sorted(decl) == sorted(bluestein.SIGS) == sorted(NAMES)
    for name, (res, args) in decl.items():
        assert bluestein.SIGS[name] == ac.signature(res, args), name
    sigs = bluestein.SIGS
    # launch_tuned = the arguments of launch + grid; benchmark = launch with the timer in the stream's place
    assert sigs["smfft_bluestein_launch_tuned"][1] == sigs["smfft_bluestein_launch"][1] + [ac.CTYPES["int"]]
    assert sigs["smfft_bluestein_benchmark"][1] == sigs["smfft_bluestein_launch"][1][:-1] + [ac.CTYPES["double*"]]
    assert bluestein.SIZES == SIZES and bluestein.MAX_LENGTH == 2048


def test_library_exports_exactly_the_seven_symbols(bluestein_lib):
    ac.check_exports(bluestein_lib, NAMES)


# ---- 6: rejections -------------------------------------------------------------------------------------------------
def test_unsupported_combinations_return_minus_one_without_a_device(bluestein_lib):
    """-1 (or 0 for an empty batch) before any HIP call: run in a process where no GPU is visible, with null pointers"""
    code = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
ll = ctypes.c_longlong
lib.smfft_bluestein_plan_bytes.restype = ll
t = ctypes.c_double(0.0)
def calls(n, batch, grid=3):
    return [lib.smfft_bluestein_launch(None, None, n, ll(batch), None, None),
            lib.smfft_bluestein_launch_tuned(None, None, n, ll(batch), None, None, grid),
            lib.smfft_bluestein_benchmark(None, None, n, ll(batch), None, ctypes.byref(t))]
rc = []
for n in (0, -5, 2049, 4096):
    rc += calls(n, 10) + calls(n, 0)
    rc += [lib.smfft_bluestein_fft_size(n), lib.smfft_bluestein_plan_bytes(n), lib.smfft_bluestein_tables(n, 0, None), lib.smfft_bluestein_prepare(n, 0, None, None)]
for n in (1, 1000, 2048):
    rc += calls(n, -1)
    for grid in (0, -1):
        rc += [lib.smfft_bluestein_launch_tuned(None, None, n, ll(10), None, None, grid), lib.smfft_bluestein_launch_tuned(None, None, n, ll(0), None, None, grid)]
empty = []
for n in (1, 128, 129, 1000, 2048):
    empty += calls(n, 0)
print(rc, empty, t.value)
sys.exit(0 if rc and rc == [-1] * len(rc) and empty == [0] * 15 and t.value == 0.0 else 1)
"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code, bluestein_lib], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stdout + p.stderr


def test_python_wrappers_refuse_before_a_device(bluestein_lib):
    from smfft_amd import bluestein
    for n in (0, -5, 2049, 4096):
        with pytest.raises(RuntimeError):
            bluestein.launch(None, None, n, 10, None)
        with pytest.raises(RuntimeError):
            bluestein.launch_tuned(None, None, n, 10, None, 3)
        with pytest.raises(RuntimeError):
            bluestein.prepare(n, None)
        assert bluestein.benchmark(None, None, n, 10, None) == (-1, 0.0)
        for fn in (bluestein.fft_size, bluestein.plan_bytes, bluestein.tables):
            with pytest.raises(ValueError):
                fn(n)
    with pytest.raises(RuntimeError):
        bluestein.launch(None, None, 1000, -1, None)
    for grid in (0, -1):
        with pytest.raises(RuntimeError):
            bluestein.launch_tuned(None, None, 1000, 10, None, grid)
    assert bluestein.benchmark(None, None, 1000, 0, None) == (0, 0.0)
    with pytest.raises(ValueError):
        bluestein.fft(np.zeros(2049, np.complex64))
    with pytest.raises(ValueError):
        bluestein.fft(np.zeros((3, 0), np.complex64))
    with pytest.raises(ValueError):
        bluestein.fft(np.complex64(1))


def test_import_does_not_load_the_library():
    ac.check_import_does_not_load("bluestein", "smfft_bluestein")

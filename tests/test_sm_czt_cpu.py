"""CPU checks of the chirp-z transforms (smfft_amd/csrc/smfft_czt.hip, libsmfft_czt.so): the fp64 model of the kernel's chain
(tools/czt_model.py) is the O(n m) sum of the definition, whose phases are exact to 1e-12 cycles; the library's host-built tables are
the model's, rounded once to fp32; the table builder runs clean under the address and undefined-behaviour sanitizers as a stand-alone
host program; the gfx950 code of the five kernels keeps the Bluestein kernels' budget; and the C ABI declares, exports and validates
the seven entry points without a device.  No GPU code is run (hipcc cross-compiles gfx950)."""
import ctypes
import fractions
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import czt_model as cm  # noqa: E402

from tests import addon_checks as ac  # noqa: E402
from tests import czt_inventory  # noqa: E402

CSRC = ac.CSRC
LIB = os.path.join(ROOT, "smfft_amd", "libsmfft_czt.so")
SIZES = (256, 512, 1024, 2048, 4096)
# (n, m, start, step)
CASES = ((1, 1, .3, .1), (5, 3, .1, .01), (128, 129, .25, 1 / 1024), (200, 57, -.2, .003), (1000, 24, .123, 1e-4), (2048, 2048, 0, 1 / 2048),
         (2048, 1, .37, 0), (1, 2048, .1, 7e-4), (300, 2048, .9, -.013), (1536, 513, .4, .3))
NAMES = ("smfft_czt_fft_size", "smfft_czt_plan_bytes", "smfft_czt_tables", "smfft_czt_prepare", "smfft_czt_launch", "smfft_czt_launch_tuned",
         "smfft_czt_benchmark")
# the transform region of 4096 points; at M >= 2048 the output chirp C, M float2, lives behind it
LDS_BYTES = {m: 4096 // 16 * 17 * 8 + (8 * m if m >= 2048 else 0) for m in SIZES}
NO_DEVICE = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


@pytest.fixture(scope="module")
def czt_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", CSRC, "-j", "4", "../libsmfft_czt.so"])
    return LIB


# ---- 1: the model -------------------------------------------------------------------------------------------
def test_model_is_the_direct_sum():
    """the chain pad, FFT_M, product with B M, IFFT_M, window with the plan's fp64 tables equals the O(n m) sum within 1e-12 of the
    largest output"""
    rng = np.random.default_rng(19)
    for n, m, start, step in CASES:
        x = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
        want = cm.direct(x, m, start, step)
        assert want.shape == (3, m)
        err = np.max(np.abs(cm.model(x, m, start, step) - want)) / np.max(np.abs(want))
        print(f"n={n} m={m} start={start} step={step}: max |model - direct| / max |direct| = {err:.2e}")
        assert err <= 1e-12, (n, m, start, step, err)


@pytest.mark.parametrize("n", [1, 5, 128, 1000, 2048])
def test_direct_is_numpys_fft_on_the_dft_arc(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
    for step, want in ((1 / n, np.fft.fft(x, axis=-1)), (-1 / n, np.fft.ifft(x, axis=-1) * n)):
        err = np.max(np.abs(cm.direct(x, n, 0.0, step) - want)) / np.max(np.abs(want))
        print(f"n={n} step={step}: max |direct - numpy| / max |numpy| = {err:.2e}")
        assert err <= 1e-12, (n, step, err)


def test_direct_phases_are_exact_to_1e_12_cycles():
    """j (start + k step) mod 1 in rational arithmetic on the doubles' own values, on a sample of (j, k) that holds the corners"""
    rng = np.random.default_rng(12)
    worst = 0.0
    for n, m, start, step in CASES + ((2048, 2048, 5.25, -1.75), (2048, 2048, -123.456, 0.49999), (2048, 2048, 1e6 + .1, 1e-9)):
        got = cm.phases(n, m, start, step)
        assert got.shape == (n, m)
        fs, ft = fractions.Fraction(float(start)), fractions.Fraction(float(step))
        js = {0, n - 1, n // 2} | {int(v) for v in rng.integers(0, n, 6)}
        ks = {0, m - 1, m // 2} | {int(v) for v in rng.integers(0, m, 6)}
        for j in js:
            for k in ks:
                d = fractions.Fraction(float(got[j, k])) - j * (fs + k * ft)
                worst = max(worst, abs(float(d - round(d))))
    print(f"worst phase error: {worst:.2e} cycles")
    assert worst <= 1e-12


def test_fft_size_is_minimal_and_symmetric():
    n = np.arange(1, 2049)
    need = n[:, None] + n[None, :] - 1
    want = np.full(need.shape, 256)
    for M in SIZES[1:]:
        want[need > M // 2] = M
    assert np.all(want >= need) and np.all((want == 256) | (want // 2 < need)) and np.array_equal(want, want.T)
    for i in (1, 2, 127, 128, 129, 1000, 1024, 1025, 2047, 2048):        # whole rows of the grid through the model ...
        assert [cm.fft_size(i, int(j)) for j in n] == list(want[i - 1]), i
        assert [cm.fft_size(int(j), i) for j in n] == list(want[i - 1]), i
    for bad in ((0, 5), (5, 0), (-1, 5), (2049, 1), (1, 2049)):
        with pytest.raises(ValueError):
            cm.fft_size(*bad)
    for M, shapes in czt_inventory.SHAPES.items():
        assert all(cm.fft_size(*s) == M for s in shapes), M


def test_library_fft_size_over_the_whole_grid(czt_lib, tmp_path):
    """... and the library's own over all 2048 x 2048 shapes, in a process with no visible device"""
    code = r"""
import ctypes, sys
import numpy as np
lib = ctypes.CDLL(sys.argv[1])
f = lib.smfft_czt_fft_size
got = np.array([[f(n, m) for m in range(1, 2049)] for n in range(1, 2049)], np.int32)
np.save(sys.argv[2], got)
lib.smfft_czt_plan_bytes.restype = ctypes.c_longlong
bad = [f(n, m) for n, m in ((0, 5), (5, 0), (-1, 5), (2049, 1), (1, 2049))] + [lib.smfft_czt_plan_bytes(0, 5), lib.smfft_czt_plan_bytes(5, 2049)]
sys.exit(0 if bad == [-1] * 7 and lib.smfft_czt_plan_bytes(300, 200) == 24 * 512 else 1)
"""
    path = str(tmp_path / "sizes.npy")
    p = subprocess.run([sys.executable, "-c", code, czt_lib, path], capture_output=True, text=True, timeout=300, env=dict(os.environ, **NO_DEVICE))
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.load(path)
    n = np.arange(1, 2049)
    need = n[:, None] + n[None, :] - 1
    assert np.all(np.isin(got, SIZES)) and np.all(got >= need) and np.all((got == 256) | (got // 2 < need)) and np.array_equal(got, got.T)


# ---- 2: the tables -------------------------------------------------------------------------------------------
TABLE_CASES = CASES + ((200, 57, .25, .003), (200, 57, 5.25, .003), (200, 57, -.75, .003), (2048, 2048, .5, 1.0), (2048, 2047, -.5, 2.999))


def test_tables_are_the_models_rounded_once(czt_lib, tmp_path):
    """smfft_czt_tables in a process with no visible device, into a guarded host buffer: every component of A, B and C within
    2^-24 |value| + 1e-8 of the model's fp64 value.  The 1e-8: after the reduction of start and step the largest phase is
    2048 / 2 + 2048^2 / 2 = 2.1e6 cycles, and three fp64 roundings of that are 7e-10 cycles = 4.4e-9 rad; a builder that forms its
    phases in fp32 misses by 1e-1.  A is zero from n on and C from m on; whole cycles of start change nothing; what is not finite is
    refused"""
    code = r"""
import ctypes, sys
import numpy as np
lib = ctypes.CDLL(sys.argv[1])
d = ctypes.c_double
lib.smfft_czt_plan_bytes.restype = ctypes.c_longlong
lib.smfft_czt_tables.argtypes = [ctypes.c_int, ctypes.c_int, d, d, ctypes.c_void_p]
out = {}
for i, case in enumerate(sys.argv[3:]):
    n, m, start, step = case.split(",")
    n, m, start, step = int(n), int(m), float(start), float(step)
    M = lib.smfft_czt_fft_size(n, m)
    assert lib.smfft_czt_plan_bytes(n, m) == 24 * M
    guarded = np.full(3 * M + 64, np.complex64(7 - 7j))
    assert lib.smfft_czt_tables(n, m, start, step, guarded.ctypes.data + 8 * 32) == 0
    assert np.all(guarded[:32] == 7 - 7j) and np.all(guarded[-32:] == 7 - 7j)
    out[str(i)] = guarded[32:-32].copy()
plan = np.full(3 * 256, np.complex64(7 - 7j))
for start, step in ((float("nan"), .1), (.1, float("nan")), (float("inf"), .1), (.1, float("-inf"))):
    assert lib.smfft_czt_tables(5, 3, start, step, plan.ctypes.data) == -1
assert lib.smfft_czt_tables(5, 3, .1, .1, None) == -1
assert np.all(plan == 7 - 7j)
np.savez(sys.argv[2], **out)
"""
    path = str(tmp_path / "tables.npz")
    args = [f"{n},{m},{start!r},{step!r}" for n, m, start, step in TABLE_CASES]
    p = subprocess.run([sys.executable, "-c", code, czt_lib, path] + args, capture_output=True, text=True, timeout=300, env=dict(os.environ, **NO_DEVICE))
    assert p.returncode == 0, p.stdout + p.stderr
    got_all = np.load(path)

    def close(got, want, what):
        for g, w in ((got.real, want.real), (got.imag, want.imag)):
            excess = np.abs(g.astype(np.float64) - w) - (2.0 ** -24 * np.abs(w) + 1e-8)
            assert np.all(excess <= 0), (what, int(np.argmax(excess)), float(np.max(excess)))

    for i, (n, m, start, step) in enumerate(TABLE_CASES):
        M = cm.fft_size(n, m)
        got, want = got_all[str(i)], cm.plan(n, m, start, step)
        assert got.dtype == np.complex64 and got.shape == want.shape == (3 * M,)
        close(got, want, (n, m, start, step))
        assert not got[n:M].any() and not got[2 * M + m:].any(), (n, m)
        assert np.all(np.abs(np.abs(got[:n]) - 1) <= 1e-6) and np.all(np.abs(np.abs(got[2 * M:2 * M + m]) - 1) <= 1e-6)
    base = cm.plan(200, 57, .25, .003)
    for i, case in enumerate(TABLE_CASES):
        if case[:2] == (200, 57) and case[2] in (5.25, -.75):
            close(got_all[str(i)], base, case)


def test_mirror_tables_and_sizes(czt_lib):
    from smfft_amd import czt
    for n, m in ((1, 1), (128, 129), (1000, 24), (2048, 2048)):
        M = cm.fft_size(n, m)
        assert czt.fft_size(n, m) == M and czt.plan_bytes(n, m) == 24 * M
        t = czt.tables(n, m, .1, 1 / (8 * n))
        assert t.dtype == np.complex64 and t.shape == (3 * M,)
        # the opposite arc: A and C conjugate
        u = czt.tables(n, m, -.1, -1 / (8 * n))
        assert np.array_equal(u[:n], np.conj(t[:n])) and np.array_equal(u[2 * M:], np.conj(t[2 * M:]))


# ---- 3: the table builder under the sanitizers ---------------------------------------------------------------
SANITIZED_MAIN = r"""
#include <cstdio>
#include <vector>
#include "smfft_czt_tables.hpp"
int main() {
    const int shapes[][2] = {{1, 1}, {128, 129}, {2047, 2}, {2, 2047}, {2048, 2048}, {300, 200}, {1000, 25}, {2048, 1}, {1, 2048}};
    const double arcs[][2] = {{0.0, 1.0 / 300}, {0.1, 1.0 / 2400}, {-0.2, -0.013}, {0.37, 0.0}, {5.25, 2.999}, {-1e9, 1e300}};
    double sum = 0.0;
    for (const auto& s : shapes) {
        for (const auto& a : arcs) {
            const int M = smfft::czt::fft_size(s[0], s[1]);
            std::vector<float> plan(6 * (size_t)M);          // exactly the plan: a write past it is a heap overflow
            smfft::czt::build_tables(s[0], s[1], a[0], a[1], plan.data());
            for (float v : plan) sum += v;
        }
    }
    if (smfft::czt::fft_size(0, 1) != -1 || smfft::czt::fft_size(1, 2049) != -1 || smfft::czt::fft_size(2048, 2048) != 4096) return 2;
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
    src, exe = tmp_path / "czt_tables_main.cpp", tmp_path / "czt_tables_main"
    src.write_text(SANITIZED_MAIN)
    c = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr.strip(), p.stdout + p.stderr
    assert re.fullmatch(r"-?\d+\.\d+\n", p.stdout), p.stdout
    header = open(os.path.join(CSRC, "smfft_czt_tables.hpp")).read()
    assert "hip" not in re.sub(r"//.*", "", header).lower()      # plain C++: no HIP in the code


# ---- 4: ISA budget and inventory -------------------------------------------------------------------------------
def _loops(body):
    """per line of a kernel body, the header of the innermost loop of its basic block (None outside every loop), from the annotations the
    compiler writes behind a block's label ("in Loop: Header=BB0_6 Depth=1", "This Inner Loop Header: Depth=1")"""
    loops, loop, i = [], None, 0
    while i < len(body):
        label = re.match(r"\.L(BB\d+_\d+):", body[i])
        if label or re.match(r"; %bb\.\d+:", body[i]):
            notes, j = body[i], i + 1
            while j < len(body) and body[j].startswith(";") and not body[j].startswith("; %bb."):
                notes, j = notes + body[j], j + 1
            header = re.search(r"Header=(BB\d+_\d+)", notes)
            loop = header.group(1) if header else (label.group(1) if label and "Loop Header" in notes else None)
        loops.append(loop)
        i += 1
    return loops


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """{M: assembly of smfft_czt_<M>.o as the Makefile compiles it}"""
    if not os.path.exists(ac.HIPCC):
        pytest.skip("hipcc not installed")
    return ac.addon_isa("smfft_czt", "CZT", SIZES, tmp_path_factory.mktemp("czt_isa"))


def test_isa_budget_of_what_ships(isa):
    """per M exactly one kernel: no scratch, at most 256 VGPRs (two waves per SIMD, the Bluestein kernels' occupancy), the LDS of 4096
    points plus C at M >= 2048 with room for two workgroups per compute unit, no transcendentals, no packed f32 arithmetic; a thread's
    sixteen row loads -- the kernel's only non-temporal loads -- go out with no branch, barrier or vmcnt(0) wait between the first and
    the last; they and the sixteen stores lie in one loop, the tile loop; every table load lies in front of it"""
    total = 0
    for m, text in isa.items():
        descs = ac.descriptors(text)
        kernels = ac.pfb_kernels(text, "czt_kernel")
        assert len(descs) == 1 and set(descs) == set(kernels), (m, sorted(descs))
        total += len(descs)
        assert not re.search(r"\bscratch_", text), m
        (name, body), = kernels.items()
        assert "czt_kernelILi%dE" % m in name
        assert not [line for line in body if re.match(r"v_(sin|cos)_", line)], name
        assert not [line for line in body if re.match(r"v_pk_(add|mul|fma)_f32", line)], name
        assert ac.descriptor_field(descs, name, "private_segment_fixed_size") == 0, name
        v, lds = ac.descriptor_field(descs, name, "next_free_vgpr"), ac.descriptor_field(descs, name, "group_segment_fixed_size")
        print(f"M={m}: czt_kernel {v} VGPRs ({ac.occupancy(v)} waves per SIMD), {lds} B of LDS")
        assert lds == LDS_BYTES[m] and 2 * lds <= ac.LDS_PER_CU, (name, lds)
        assert v <= 256 and ac.occupancy(v) >= 2, (name, v)
        loads = [i for i, line in enumerate(body) if line.startswith("global_load") and re.search(r"\bnt\b", line)]
        assert len(loads) == 16 and all(re.match(r"global_load_dwordx2\s", body[i]) for i in loads), (name, len(loads))
        between = body[loads[0]:loads[-1] + 1]
        assert not [line for line in between if line.startswith(("s_cbranch", "s_branch", "s_setpc", "s_barrier"))], name
        assert not [line for line in between if re.search(r"vmcnt\(0\)", line)], name
        stores = [i for i, line in enumerate(body) if line.startswith("global_store")]
        assert len(stores) == 16 and all(re.match(r"global_store_dwordx2\s", body[i]) and re.search(r"\bnt\b", body[i]) for i in stores), (name, len(stores))
        # the tile loop: the one loop that holds the row loads, and the stores with them; the tables' loads (and at M >= 2048 the loop
        # that stages C in LDS) lie in front of it
        loop = _loops(body)
        tile = {loop[i] for i in loads}
        assert len(tile) == 1 and None not in tile and {loop[i] for i in stores} == tile, (name, tile)
        tables = [i for i, line in enumerate(body) if line.startswith("global_load") and not re.search(r"\bnt\b", line)]
        assert len(tables) >= (33 if m >= 2048 else 48) and not ({loop[i] for i in tables} & tile) and max(tables) < loads[0], (name, len(tables))
    assert total == 5


def test_library_ships_five_kernels_and_the_inventory_names_them(czt_lib):
    ac.check_inventory(czt_lib, czt_inventory.KERNELS, "smfft_czt_", 5, kinds=("tests", "bounds", "probes"))
    assert "permlane" in czt_inventory.__doc__ and "hostsim" in czt_inventory.__doc__


# ---- 5: declarations and exports ---------------------------------------------------------------------------------
def _signature(res, args):
    """ac.signature with the doubles of this header's start and step"""
    table = dict(ac.CTYPES, double=ctypes.c_double)
    return table[res], [table[re.sub(r"\s*\w+$", "", a.strip())] for a in args.split(",")]


def test_python_mirror_matches_header(czt_lib):
    from smfft_amd import czt
    header = re.sub(r"[\s*]+", " ", open(os.path.join(ROOT, "include", "smfft_czt.h")).read())
    for phrase in ("Out of scope", "|a| != 1 or |w| != 1", "n > 2048 or m > 2048", "real input", "strided or transposed rows", "d_out == d_in",
                   "only when m == n", "rounded once to fp32", "UN-normalised", "every output element is written exactly once",
                   "Rows do not see each other", "only in[0, batch n), out[0, batch m) and the plan's 3M float2 are touched"):
        assert phrase in header, phrase
    decl = ac.declarations("smfft_czt.h")
    assert sorted(decl) == sorted(czt.SIGS) == sorted(NAMES)
    for name, (res, args) in decl.items():
        assert czt.SIGS[name] == _signature(res, args), name
    sigs = czt.SIGS
    # launch_tuned = the arguments of launch + grid; benchmark = launch with the timer in the stream's place
    assert sigs["smfft_czt_launch_tuned"][1] == sigs["smfft_czt_launch"][1] + [ac.CTYPES["int"]]
    assert sigs["smfft_czt_benchmark"][1] == sigs["smfft_czt_launch"][1][:-1] + [ac.CTYPES["double*"]]
    assert czt.SIZES == SIZES and czt.MAX_LENGTH == 2048


def test_library_exports_exactly_the_seven_symbols(czt_lib):
    ac.check_exports(czt_lib, NAMES)


# ---- 6: rejections -------------------------------------------------------------------------------------------------
def test_unsupported_combinations_return_minus_one_without_a_device(czt_lib):
    """-1 (or 0 for an empty batch) before any HIP call: run in a process where no GPU is visible, with null pointers -- which are equal,
    so d_out == d_in: refused with m != n, whatever the batch -- and with two addresses that are never read"""
    code = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
ll, d, vp, i = ctypes.c_longlong, ctypes.c_double, ctypes.c_void_p, ctypes.c_int
lib.smfft_czt_plan_bytes.restype = ll
lib.smfft_czt_tables.argtypes = [i, i, d, d, vp]
lib.smfft_czt_prepare.argtypes = [i, i, d, d, vp, vp]
head = [vp, vp, i, i, ll, vp]
lib.smfft_czt_launch.argtypes = head + [vp]
lib.smfft_czt_launch_tuned.argtypes = head + [vp, i]
lib.smfft_czt_benchmark.argtypes = head + [ctypes.POINTER(d)]
t = d(0.0)
def calls(n, m, batch, grid=3, din=None, dout=None):
    return [lib.smfft_czt_launch(din, dout, n, m, batch, None, None),
            lib.smfft_czt_launch_tuned(din, dout, n, m, batch, None, None, grid),
            lib.smfft_czt_benchmark(din, dout, n, m, batch, None, ctypes.byref(t))]
rc = []
for n, m in ((0, 5), (5, 0), (-5, 5), (5, -5), (2049, 1), (1, 2049), (4096, 4096)):
    rc += calls(n, m, 10) + calls(n, m, 0) + calls(n, m, 10, din=4096, dout=8192)
    rc += [lib.smfft_czt_fft_size(n, m), lib.smfft_czt_plan_bytes(n, m), lib.smfft_czt_tables(n, m, .1, .1, None), lib.smfft_czt_prepare(n, m, .1, .1, None, None)]
for n, m in ((1, 1), (1000, 1000), (2048, 2048), (300, 200)):
    rc += calls(n, m, -1, din=4096, dout=8192)
    for grid in (0, -1):
        rc += [lib.smfft_czt_launch_tuned(4096, 8192, n, m, 10, None, None, grid), lib.smfft_czt_launch_tuned(4096, 8192, n, m, 0, None, None, grid)]
# in place with m != n: null == null, and one real address twice
for n, m in ((300, 200), (200, 300), (2048, 1), (1, 2)):
    rc += calls(n, m, 10) + calls(n, m, 0) + calls(n, m, 10, din=4096, dout=4096)
nan, inf = float("nan"), float("inf")
for start, step in ((nan, .1), (.1, nan), (inf, .1), (.1, -inf)):
    rc += [lib.smfft_czt_tables(5, 3, start, step, None), lib.smfft_czt_prepare(5, 3, start, step, None, None)]
rc += [lib.smfft_czt_tables(5, 3, .1, .1, None)]
empty = []
for n, m in ((1, 1), (128, 128), (1000, 1000), (2048, 2048)):
    empty += calls(n, m, 0)                                    # in place, m == n
for n, m in ((128, 129), (1000, 24), (1, 2048)):
    empty += calls(n, m, 0, din=4096, dout=8192)
print(rc, empty, t.value)
sys.exit(0 if rc and rc == [-1] * len(rc) and empty == [0] * 21 and t.value == 0.0 else 1)
"""
    p = subprocess.run([sys.executable, "-c", code, czt_lib], capture_output=True, text=True, timeout=120, env=dict(os.environ, **NO_DEVICE))
    assert p.returncode == 0, p.stdout + p.stderr


def test_python_wrappers_refuse_before_a_device(czt_lib):
    from smfft_amd import czt
    for n, m in ((0, 5), (5, 0), (-5, 5), (2049, 1), (1, 2049)):
        with pytest.raises(RuntimeError):
            czt.launch(4096, 8192, n, m, 10, None)
        with pytest.raises(RuntimeError):
            czt.launch_tuned(4096, 8192, n, m, 10, None, 3)
        with pytest.raises(RuntimeError):
            czt.prepare(n, m, .1, .1, None)
        assert czt.benchmark(4096, 8192, n, m, 10, None) == (-1, 0.0)
        for fn in (czt.fft_size, czt.plan_bytes):
            with pytest.raises(ValueError):
                fn(n, m)
        with pytest.raises(ValueError):
            czt.tables(n, m, .1, .1)
    with pytest.raises(RuntimeError):
        czt.launch(4096, 8192, 1000, 24, -1, None)
    with pytest.raises(RuntimeError):
        czt.launch(4096, 4096, 1000, 24, 10, None)               # in place with m != n
    for grid in (0, -1):
        with pytest.raises(RuntimeError):
            czt.launch_tuned(4096, 8192, 1000, 24, 10, None, grid)
    assert czt.benchmark(4096, 8192, 1000, 24, 0, None) == (0, 0.0)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(RuntimeError):
            czt.prepare(5, 3, bad, .1, None)
        with pytest.raises(ValueError):
            czt.tables(5, 3, .1, bad)
        with pytest.raises(ValueError):
            czt.czt(np.zeros(5, np.complex64), start=bad)
        with pytest.raises(ValueError):
            czt.czt(np.zeros(5, np.complex64), step=bad)
    with pytest.raises(ValueError):
        czt.czt(np.zeros(2049, np.complex64))
    with pytest.raises(ValueError):
        czt.czt(np.zeros(5, np.complex64), m=2049)
    with pytest.raises(ValueError):
        czt.czt(np.zeros(5, np.complex64), m=0)
    with pytest.raises(ValueError):
        czt.czt(np.zeros((3, 0), np.complex64))
    with pytest.raises(ValueError):
        czt.czt(np.complex64(1))


def test_import_does_not_load_the_library():
    ac.check_import_does_not_load("czt", "smfft_czt")

"""CPU checks of the overlap-save FIR filter banks with N = 8192 / 16384 segments (include/smfft/smfft_large_fir.hpp,
libsmfft_large_fir.so): the fp64 model of the plan (tools/large_fir_model.py) is np.convolve / np.correlate and its store windows tile
the output once, smfft::FirWindow compiled for the host gives the model's windows at these lengths, the gfx950 code of every kernel --
the ones the library ships and the other form of the filter loop, compiled from the header -- keeps the budgets of DESIGN.md section 11,
and the C ABI declares, exports and validates the entry points without a device.  No GPU code is run (hipcc cross-compiles gfx950)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import large_fir_model as lfm  # noqa: E402

from tests import addon_checks as ac  # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "smfft_amd", "csrc")
LIB = os.path.join(ROOT, "smfft_amd", "libsmfft_large_fir.so")
SIZES = (8192, 16384)
NAMES = ac.fir_names("smfft_large_fir")
LDS_BYTES = {8192: 8 * 16 * (8192 // 16 + 2), 16384: 8 * 16 * (16384 // 16 + 2)}      # LargeGeometry<N>::kLdsBytes
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def fir_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", CSRC, "-j", "4", "../libsmfft_large_fir.so"])
    return LIB


# ---- the model ---------------------------------------------------------------------------------------
_taps_cases, _length_cases = ac.fir_taps_cases, ac.fir_length_cases


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("correlate", [False, True])
def test_model_is_numpys_convolution_and_correlation(n, correlate):
    """the plan replayed per thread (register positions u + T*q at the load, the product and the store) on the engine's model"""
    rng = np.random.default_rng(n + correlate)
    for m, length in ((17, 2 * n + 5), (n // 4 + 1, n), (n - 1, 7)):
        h = rng.standard_normal((2, m)) + 1j * rng.standard_normal((2, m))
        x = rng.standard_normal((2, length)) + 1j * rng.standard_normal((2, length))
        want = lfm.direct(x, h, correlate)
        got = lfm.overlap_save(x, h, n, correlate)
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (n, m, length, correlate)


def test_model_windows_tile_the_output_once_and_loads_stay_in_range():
    for n in SIZES:
        pos = lfm.thread_positions(n)
        assert np.array_equal(np.sort(pos.reshape(-1)), np.arange(n))
        for m in _taps_cases(n):
            for length in _length_cases(n, m):
                for corr in (False, True):
                    w = lfm.Window(length, n, m, corr)
                    covered = np.zeros(length, np.int64)
                    for s in range(w.segments()):
                        b, e = w.store_window(s)
                        assert b == m - 1 and b < e <= n
                        lo, hi = w.load_bounds(s)
                        a = w.load_start(s)
                        assert 0 <= a + lo and a + hi <= length and (lo == 0 or a + lo == 0) and (hi == n or a + hi == length)
                        stored = pos[(pos >= b) & (pos < e)]
                        covered[w.output_index(s, 0) + stored] += 1
                    assert np.all(covered == 1), (n, m, length, corr)


# ---- FirWindow through a host compile --------------------------------------------------------------------
@needs_hipcc
def test_header_window_is_the_models(tmp_path):
    cases = [(n, m, length) for n in SIZES for m in _taps_cases(n) for length in _length_cases(n, m)]
    cases += [(8192, 2049, (1 << 24)), (16384, 4097, (1 << 34) + 3)]
    src = tmp_path / "large_fir_window.hip"
    src.write_text(r'''
#include <cstdio>
#include "smfft_fir.hpp"
int main() {
    int n, m, corr; long long L;
    while (scanf("%d %d %lld %d", &n, &m, &L, &corr) == 4) {
        const smfft::FirWindow w{L, n, m, corr};
        const long long S = w.segments();
        printf("S %lld\n", S);
        const long long probe[6] = {0, 1, 2, S / 2, S - 2, S - 1};
        for (long long s : probe) {
            if (s < 0 || s >= S) continue;
            printf("%lld %lld %d %d %lld\n", s, w.load_start(s), w.store_begin(), w.store_end(s), w.output_index(s, 0));
        }
    }
    return 0;
}
''')
    exe = tmp_path / "large_fir_window"
    subprocess.check_call([HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I" + CSRC, str(src), "-o", str(exe)], stderr=subprocess.DEVNULL)
    stdin = "".join(f"{n} {m} {length} {corr}\n" for n, m, length in cases for corr in (0, 1))
    out = subprocess.run([str(exe)], input=stdin, capture_output=True, text=True, check=True).stdout.split("\n")
    want = []
    for n, m, length in cases:
        for corr in (0, 1):
            w = lfm.Window(length, n, m, corr)
            S = w.segments()
            want.append(f"S {S}")
            for s in (0, 1, 2, S // 2, S - 2, S - 1):
                if 0 <= s < S:
                    b, e = w.store_window(s)
                    want.append(f"{s} {w.load_start(s)} {b} {e} {w.output_index(s, 0)}")
    assert [line for line in out if line] == want


# ---- ISA ---------------------------------------------------------------------------------------------------
FIR_ARGS = "PK15HIP_vector_typeIfLj2EES5_PS3_NS_9FirWindowEiixNS0_14LargeFirStrideE"
PREPARE_ARGS = "PK15HIP_vector_typeIfLj2EEiiiPS3_"


def _fir_name(n, held):
    return f"_ZN5smfft5large9large_firILi{n}ELi{held}EEEv{FIR_ARGS}"


def _prepare_name(n):
    return f"_ZN5smfft5large17large_fir_prepareILi{n}EEEv{PREPARE_ARGS}"


def _compile(tmp_path, src, n, extra, tag):
    """src as the Makefile compiles the object of length n: -I. and LARGE_FIR_FLAGS_<n>"""
    return ac.device_asm(src, ["-I" + CSRC] + ac.makefile_flags("LARGE_FIR", n) + extra, tmp_path / f"{tag}.s")


def _check_kernel(text, name, n, vgpr_cap, fir):
    descs = ac.descriptors(text)
    field = lambda key: ac.descriptor_field(descs, name, key)  # noqa: E731
    body = re.search(r"^%s:[^\n]*\n(.*?)\n\s*s_endpgm" % re.escape(name), text, re.S | re.M)
    assert body, name
    lines = [line.strip() for line in body.group(1).split("\n")]
    assert field("private_segment_fixed_size") == 0, name
    assert not [line for line in lines if line.startswith("scratch_")], name
    assert field("group_segment_fixed_size") == LDS_BYTES[n], name
    vgprs = field("next_free_vgpr")
    assert vgprs <= vgpr_cap, (name, vgprs)
    assert not [line for line in lines if re.match(r"v_(sin|cos)_", line)], name
    assert not [line for line in lines if re.match(r"v_pk_(add|mul|fma)_f32", line)], name
    if fir:
        # the sixteen segment loads are the kernel's first sixteen global loads: no branch, barrier or vmcnt(0) wait among them
        loads = [i for i, line in enumerate(lines) if line.startswith("global_load")]
        assert len(loads) >= 16, name
        between = lines[loads[0]:loads[15] + 1]
        assert not [line for line in between if line.startswith(("s_cbranch", "s_branch", "s_setpc", "s_barrier"))], name
        assert not [line for line in between if re.search(r"vmcnt\(0\)", line)], name
        assert len([line for line in lines if line.startswith("s_barrier")]) == 12, name      # forward + one inverse in the loop body
    return vgprs


@needs_hipcc
@pytest.mark.parametrize("n", SIZES)
def test_isa_budget_of_what_ships(tmp_path, n):
    """the object of length n as the Makefile compiles it: the recompute form, the prepare kernel and, at 8192, the held form"""
    text = _compile(tmp_path, os.path.join(CSRC, "smfft_large_fir.hip"), n, [f"-DSMFFT_LARGE_FIR_N={n}"], f"large_fir_{n}")
    kernels = re.findall(r"\.amdhsa_kernel (\S+)", text)
    assert sorted(kernels) == sorted([_fir_name(n, 0), _prepare_name(n)] + ([_fir_name(n, 1)] if n == 8192 else []))
    v = _check_kernel(text, _fir_name(n, 0), n, 128, True)
    if n == 8192:
        vh = _check_kernel(text, _fir_name(n, 1), n, 256, True)
        assert f"`large_fir<8192, 1>` | {vh} |" in open(os.path.join(ROOT, "DESIGN.md")).read(), "DESIGN.md section 11 states another register count"
    vp = _check_kernel(text, _prepare_name(n), n, 128, False)
    print(f"N={n}: large_fir<{n}, 0> {v} VGPRs, large_fir_prepare<{n}> {vp} VGPRs")
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert f"`large_fir<{n}, 0>` | {v} |" in design and f"`large_fir_prepare<{n}>` | {vp} |" in design, "DESIGN.md section 11 states other register counts"
    assert not re.search(r"\bscratch_", text)


@needs_hipcc
def test_isa_budget_of_the_held_form(tmp_path):
    """the held form compiled from the header alone (it exists at 8192 only): one workgroup per CU, so 256 VGPRs; no scratch"""
    src = tmp_path / "held.hip"
    src.write_text('#include "smfft/smfft_large_fir.hpp"\n'
                   "template __global__ void smfft::large::large_fir<8192, 1>(const float2*, const float2*, float2*, smfft::FirWindow, int, int, long long,\n"
                   "                                                          smfft::large::LargeFirStride);\n")
    text = _compile(tmp_path, src, 8192, [], "held")
    assert re.findall(r"\.amdhsa_kernel (\S+)", text) == [_fir_name(8192, 1)]
    v = _check_kernel(text, _fir_name(8192, 1), 8192, 256, True)
    print(f"large_fir<8192, 1> {v} VGPRs")
    assert f"`large_fir<8192, 1>` | {v} |" in open(os.path.join(ROOT, "DESIGN.md")).read(), "DESIGN.md section 11 states another register count"


def test_shipped_library_holds_these_kernels(fir_lib):
    """recompute at both lengths, held at 8192 (what launches of K > 1 use there: DESIGN.md section 11), the two prepare kernels"""
    from tests import test_kernel_inventory as kinv
    handles, stubs = kinv._shipped_kernels(fir_lib)
    assert handles == stubs and len(handles) == 5, sorted(handles)
    for want in ("large_fir<8192, 0>", "large_fir<8192, 1>", "large_fir<16384, 0>", "large_fir_prepare<8192>", "large_fir_prepare<16384>"):
        assert [k for k in handles if want in k], (want, sorted(handles))


# ---- C ABI and Python mirror ---------------------------------------------------------------------------------
def test_python_mirror_matches_header(fir_lib):
    from smfft_amd import large_fir
    decl = ac.declarations("smfft_large_fir.h")
    assert sorted(decl) == sorted(large_fir.SIGS) == sorted(NAMES)
    for name, (res, args) in decl.items():
        assert res == "int" and large_fir.SIGS[name] == ac.signature(res, args), name
    assert large_fir.SIZES == SIZES
    # the declarations are those of the FIR block of include/smfft.h, word for word, under the new names
    base = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smfft.h")).read(), flags=re.S)
    for name, (_, args) in decl.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name.replace("smfft_large_fir_", "smfft_fir_"), base)
        assert m and re.sub(r"\s+", " ", m.group(1)) == re.sub(r"\s+", " ", args), name


def test_library_exports_exactly_the_three_symbols(fir_lib):
    nm = subprocess.run(["nm", "-D", "--defined-only", fir_lib], capture_output=True, text=True, check=True).stdout
    exported = sorted(re.findall(r" T (smfft_\w+)$", nm, re.M))
    assert exported == sorted(NAMES)


def test_unsupported_combinations_return_minus_one_without_a_device(fir_lib):
    """-1 (or 0 for an empty signal) before any HIP call: run in a process where no GPU is visible, with null pointers"""
    ac.check_fir_rejections(fir_lib, "smfft_large_fir", SIZES)


def test_python_wrappers_refuse_before_a_device(fir_lib):
    from smfft_amd import large_fir
    ac.check_fir_wrappers_refuse(large_fir.prepare, large_fir.launch, SIZES)


def test_default_fft_size_rule():
    """fft_size=None: N = clamp(next_pow2(4 M), 8192, 16384), the rule of smfft_amd.fir carried up; M >= 16384 is refused before
    anything touches a device; smfft_amd.fir keeps its own limit"""
    import smfft_amd
    from smfft_amd import large_fir
    for m, n in ((1, 8192), (17, 8192), (2048, 8192), (2049, 16384), (4097, 16384), (8192, 16384), (16383, 16384)):
        assert large_fir.fir_fft_size(m) == n == lfm.fft_size(m), m
    for m in (0, 16384, 20000):
        with pytest.raises(ValueError):
            large_fir.fir_fft_size(m)
    with pytest.raises(ValueError):
        large_fir.fir(np.zeros(10, np.complex64), np.zeros(16384, np.complex64))
    with pytest.raises(ValueError):
        large_fir.fir(np.zeros(10, np.complex64), np.zeros(17, np.complex64), fft_size=4096)
    with pytest.raises(ValueError):
        smfft_amd.fir(np.zeros(10, np.complex64), np.zeros(4096, np.complex64))


def test_import_does_not_load_the_library():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import smfft_amd, smfft_amd.large_fir as l; assert l._lib is None; "
            "maps = open('/proc/self/maps').read(); assert 'libsmfft_large_fir' not in maps; print('ok')")
    p = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout + p.stderr

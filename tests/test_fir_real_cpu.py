"""CPU checks of the overlap-save FIR filter banks for real signals and real taps (smfft_amd/csrc/smfft_fir_real.hip,
libsmfft_fir_real.so): the fp64 model of the plan (tools/fir_real_model.py) is np.convolve / np.correlate, the store windows of its
pairs tile the output once and its loads stay inside the channel, smfft::FirPairs compiled for the host gives the model's numbers, the
gfx950 code of every kernel keeps the budgets of DESIGN.md section 16 and the occupancy of the complex bank's kernel, and the C ABI
declares, exports and validates the entry points without a device.  No GPU code is run (hipcc cross-compiles gfx950)."""
import concurrent.futures
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fir_real_model as frm  # noqa: E402

from tests import addon_checks as ac  # noqa: E402
from tests import fir_real_inventory  # noqa: E402

HIPCC = ac.HIPCC
CSRC = ac.CSRC
LIB = os.path.join(ROOT, "smfft_amd", "libsmfft_fir_real.so")
SIZES = (256, 512, 1024, 2048, 4096)
NAMES = ac.fir_names("smfft_fir_real")
LDS_BYTES = 4096 // 16 * 17 * 8
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def fir_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", CSRC, "-j", "4", "../libsmfft_fir_real.so"])
    return LIB


# ---- the model ---------------------------------------------------------------------------------------
_taps_cases, _length_cases = ac.fir_taps_cases, ac.fir_length_cases


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("correlate", [False, True])
def test_model_is_numpys_convolution_and_correlation(n, correlate):
    """the plan replayed per thread (register positions u + T*q at the two loads, the product and the two stores) in fp64"""
    rng = np.random.default_rng(n + correlate)
    worst = 0.0
    for m in _taps_cases(n):
        for length in _length_cases(n, m):
            if length < 1:
                continue
            x, h = rng.standard_normal((2, length)), rng.standard_normal((2, m))
            want = frm.direct(x, h, correlate)
            assert np.all(want.imag == 0)
            got = frm.overlap_save_pairs(x, h, n, correlate)
            err = np.max(np.abs(got - want.real)) / np.max(np.abs(want))
            worst = max(worst, err)
            assert err <= 1e-12, (n, m, length, correlate, err)
    print(f"N={n} correlate={correlate}: max |model - numpy| / max |numpy| = {worst:.2e}")


def test_store_windows_tile_the_output_once_and_loads_stay_in_range():
    for n in SIZES:
        pos = frm.thread_positions(n)
        assert np.array_equal(np.sort(pos.reshape(-1)), np.arange(n))
        for m in _taps_cases(n):
            for length in _length_cases(n, m):
                if length < 1:
                    continue
                for corr in (False, True):
                    pr = frm.Pairs(length, n, m, corr)
                    S, P = pr.w.segments(), pr.pairs()
                    assert P == -(-S // 2)
                    covered = np.zeros(length, np.int64)
                    for p in range(P):
                        assert pr.present(p, 0) and pr.present(p, 1) == (2 * p + 1 < S)
                        for lane in (0, 1):
                            e = pr.store_end(p, lane)
                            if not pr.present(p, lane):
                                assert e == 0                       # an absent partner stores nothing
                                continue
                            assert m - 1 < e <= n
                            lo, hi = pr.load_bounds(p, lane)
                            a = pr.load_start(p, lane)
                            assert 0 <= a + lo and a + hi <= length and (lo == 0 or a + lo == 0) and (hi == n or a + hi == length)
                            stored = pos[(pos >= m - 1) & (pos < e)]
                            covered[pr.output_index(p, lane, 0) + stored] += 1
                        assert pr.load_start(p, 1) - pr.load_start(p, 0) == pr.w.V == pr.output_index(p, 1, 0) - pr.output_index(p, 0, 0)
                        b, e = pr.load_range(p)
                        assert 0 <= b < e <= length
                    assert np.all(covered == 1), (n, m, length, corr)


def test_nan_footprint_is_the_union_of_the_pairs_that_read_the_sample():
    """a sample in the overlap of two pairs reaches both, one in a lone last segment or in a pair's second segment reaches that pair"""
    n, m = 256, 65
    v = n - m + 1
    length = 5 * v - 3                                       # S = 5: pairs (0, 1), (2, 3) and a lone segment 4
    pr = frm.Pairs(length, n, m, False)
    assert pr.w.segments() == 5 and pr.pairs() == 3 and not pr.present(2, 1)
    both = frm.nan_footprint(length, n, m, False, 2 * v - 1)          # the last M - 1 samples of pair 0 are the history of pair 1
    assert both[:4 * v].all() and not both[4 * v:].any()
    lone = frm.nan_footprint(length, n, m, False, length - 1)
    assert lone[4 * v:].all() and not lone[:4 * v].any()
    second = frm.nan_footprint(length, n, m, False, v + 10)           # inside segment 1 only: segment 0's outputs are hit, pair 1's not
    assert second[:2 * v].all() and not second[2 * v:].any()


# ---- FirPairs through a host compile --------------------------------------------------------------------
@needs_hipcc
def test_header_pairs_are_the_models(tmp_path):
    cases = [(n, m, length) for n in SIZES for m in _taps_cases(n) for length in _length_cases(n, m) if length >= 1]
    cases += [(1024, 257, 1 << 24), (4096, 1025, (1 << 34) + 3), (256, 255, (1 << 34) + 3)]
    src = tmp_path / "fir_real_pairs.hip"
    src.write_text(r'''
#include <cstdio>
#include "smfft_fir_real.hpp"
int main() {
    int n, m, corr; long long L;
    while (scanf("%d %d %lld %d", &n, &m, &L, &corr) == 4) {
        const smfft::FirPairs fp{smfft::FirWindow{L, n, m, corr}};
        const long long P = fp.pairs();
        printf("P %lld\n", P);
        const long long probe[6] = {0, 1, 2, P / 2, P - 2, P - 1};
        for (long long p : probe) {
            if (p < 0 || p >= P) continue;
            for (int lane = 0; lane < 2; ++lane)
                printf("%lld %d %d %lld %d %lld\n", p, lane, (int)fp.present(p, lane), fp.load_start(p, lane), fp.store_end(p, lane), fp.output_index(p, lane, 0));
        }
    }
    return 0;
}
''')
    exe = tmp_path / "fir_real_pairs"
    subprocess.check_call([HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I" + CSRC, str(src), "-o", str(exe)], stderr=subprocess.DEVNULL)
    stdin = "".join(f"{n} {m} {length} {corr}\n" for n, m, length in cases for corr in (0, 1))
    out = subprocess.run([str(exe)], input=stdin, capture_output=True, text=True, check=True).stdout.split("\n")
    want = []
    for n, m, length in cases:
        for corr in (0, 1):
            pr = frm.Pairs(length, n, m, corr)
            P = pr.pairs()
            want.append(f"P {P}")
            for p in (0, 1, 2, P // 2, P - 2, P - 1):
                if 0 <= p < P:
                    for lane in (0, 1):
                        want.append(f"{p} {lane} {int(pr.present(p, lane))} {pr.load_start(p, lane)} {pr.store_end(p, lane)} {pr.output_index(p, lane, 0)}")
    assert [line for line in out if line] == want


# ---- ISA ---------------------------------------------------------------------------------------------------
def _bodies(text, frag):
    found = {}
    for m in re.finditer(r"^(_Z\w*%s\w*):[^\n]*\n(.*?)\n\s*s_endpgm" % frag, text, re.S | re.M):
        found[m.group(1)] = [line.strip() for line in m.group(2).split("\n")]
    return found


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """{N: assembly of smfft_fir_real_<N>.o as the Makefile compiles it}, and the assembly of the main library's smfft_fir.hip"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    tmp = tmp_path_factory.mktemp("fir_real_isa")

    def compile_one(n):
        if n == 0:
            return ac.device_asm(os.path.join(CSRC, "smfft_fir.hip"), [], tmp / "smfft_fir.s")
        return ac.device_asm(os.path.join(CSRC, "smfft_fir_real.hip"), ["-I" + CSRC] + ac.makefile_flags("FIR_REAL", n) + [f"-DSMFFT_FIR_REAL_N={n}"],
                             tmp / f"smfft_fir_real_{n}.s")
    with concurrent.futures.ThreadPoolExecutor(6) as pool:
        texts = list(pool.map(compile_one, SIZES + (0,)))
    return dict(zip(SIZES, texts[:-1])), texts[-1]


def test_isa_budget_of_what_ships(isa):
    """per length exactly two kernels: no scratch, the LDS of 4096 points, no transcendentals, no packed f32 arithmetic; the 32 signal
    loads of a pair -- the kernel's only one-dword loads; the spectra come in as dwordx2 -- go out with no branch, barrier or vmcnt(0)
    wait between the first and the last, inside the tile loop and in front of the filter loop; the registers are those DESIGN.md section 16 states and allow the occupancy of the complex
    bank's fir_overlap_save_kernel<N>, compiled here from smfft_fir.hip with the main library's flags"""
    real, cplx = isa
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    cdescs = ac.descriptors(cplx)
    total = 0
    for n, text in real.items():
        descs = ac.descriptors(text)
        fir, prep = _bodies(text, "fir_real_overlap_save_kernel"), _bodies(text, "fir_real_prepare_kernel")
        assert len(descs) == 2 and len(fir) == 1 and len(prep) == 1 and set(descs) == set(fir) | set(prep), (n, sorted(descs))
        total += len(descs)
        assert not re.search(r"\bscratch_", text), n
        for name, body in {**fir, **prep}.items():
            assert "ILi%dE" % n in name
            assert not [line for line in body if line.startswith("scratch_")], name
            assert not [line for line in body if re.match(r"v_(sin|cos)_", line)], name
            assert not [line for line in body if re.match(r"v_pk_(add|mul|fma)_f32", line)], name
            assert ac.descriptor_field(descs, name, "private_segment_fixed_size") == 0, name
            assert ac.descriptor_field(descs, name, "group_segment_fixed_size") == LDS_BYTES, name
        (fname, fbody), (pname, _) = next(iter(fir.items())), next(iter(prep.items()))
        loads = [i for i, line in enumerate(fbody) if re.match(r"global_load_dword\s", line)]
        assert len(loads) == 32, (fname, len(loads))
        assert fbody.index(next(line for line in fbody if line.startswith("global_load"))) < loads[0]      # (the first filter's spectrum)
        between = fbody[loads[0]:loads[-1] + 1]
        assert not [line for line in between if line.startswith(("s_cbranch", "s_branch", "s_setpc", "s_barrier"))], fname
        assert not [line for line in between if re.search(r"vmcnt\(0\)", line)], fname
        assert not [line for line in between if line.startswith("global_load") and not re.match(r"global_load_dword\s", line)], fname
        # the loads sit in the tile loop (a label in front of them is the target of a branch behind them) and not in the filter loop
        # (a backward branch around the 32 stores whose target lies behind the loads)
        labels = {line.split(":")[0]: i for i, line in enumerate(fbody) if re.match(r"\.LBB\d+_\d+:", line)}
        back = [(labels[line.split()[-1]], i) for i, line in enumerate(fbody) if line.startswith(("s_cbranch", "s_branch")) and labels.get(line.split()[-1], i) < i]
        store_at = [j for j, line in enumerate(fbody) if line.startswith("global_store")]
        assert [1 for t, i in back if t < loads[0] and i > loads[-1]], (fname, back)
        assert [1 for t, i in back if loads[-1] < t < store_at[0] and i > store_at[-1]], (fname, back)
        # the two stores of an element are dword vector stores, 32 per filter
        stores = [line for line in fbody if line.startswith("global_store")]
        assert len(stores) == 32 and all(re.match(r"global_store_dword\s", line) for line in stores), fname
        v, vp = ac.descriptor_field(descs, fname, "next_free_vgpr"), ac.descriptor_field(descs, pname, "next_free_vgpr")
        cname = next(k for k in cdescs if "fir_overlap_save_kernelILi%dE" % n in k)
        vc = ac.descriptor_field(cdescs, cname, "next_free_vgpr")
        print(f"N={n}: fir_real_overlap_save_kernel {v} VGPRs (complex bank: {vc}), fir_real_prepare_kernel {vp} VGPRs, {LDS_BYTES} B of LDS")
        assert ac.occupancy(v) >= ac.occupancy(vc), (n, v, vc)
        assert f"`fir_real_overlap_save_kernel<{n}>` | {v} |" in design and f"`fir_real_prepare_kernel<{n}>` | {vp} |" in design, \
            f"DESIGN.md section 16 states other register counts than {v} / {vp} at N = {n}"
    assert total == 10


def test_library_ships_ten_kernels_and_the_inventory_names_them(fir_lib):
    ac.check_inventory(fir_lib, fir_real_inventory.KERNELS, "smfft_fir_real_", 10, kinds=("tests", "bounds", "probes"))
    assert "permlane" in fir_real_inventory.__doc__ and "hostsim" in fir_real_inventory.__doc__


# ---- C ABI and Python mirror ---------------------------------------------------------------------------------
def test_python_mirror_matches_header(fir_lib):
    from smfft_amd import fir_real
    header = re.sub(r"[\s*]+", " ", open(os.path.join(ROOT, "include", "smfft_fir_real.h")).read())
    for phrase in ("Out of scope", "complex taps on real signals", "N >= 8192", "PAIR", "may be passed to either launch", "neither exploits nor"):
        assert phrase in header, phrase
    decl = ac.declarations("smfft_fir_real.h")
    assert sorted(decl) == sorted(fir_real.SIGS) == sorted(NAMES)
    for name, (res, args) in decl.items():
        assert res == "int" and fir_real.SIGS[name] == ac.signature(res, args), name
    assert fir_real.SIZES == SIZES
    # the declarations are those of the FIR block of include/smfft.h, word for word, under the new names
    base = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smfft.h")).read(), flags=re.S)
    for name, (_, args) in decl.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name.replace("smfft_fir_real_", "smfft_fir_"), base)
        assert m and re.sub(r"\s+", " ", m.group(1)) == re.sub(r"\s+", " ", args), name


def test_library_exports_exactly_the_three_symbols(fir_lib):
    nm = subprocess.run(["nm", "-D", "--defined-only", fir_lib], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r" T (smfft_\w+)$", nm, re.M)) == sorted(NAMES)


def test_unsupported_combinations_return_minus_one_without_a_device(fir_lib):
    """-1 (or 0 for an empty signal) before any HIP call: run in a process where no GPU is visible, with null pointers"""
    ac.check_fir_rejections(fir_lib, "smfft_fir_real", SIZES)


def test_python_wrappers_refuse_before_a_device(fir_lib):
    from smfft_amd import fir_real
    ac.check_fir_wrappers_refuse(fir_real.prepare, fir_real.launch, SIZES)
    assert fir_real.benchmark(None, 1000, 1, None, 1, 17, 8192, None) == (-1, 0.0)
    # complex input is refused, never stripped of its imaginary part
    for x, h in ((np.zeros(10, np.complex64), np.zeros(17, np.float32)), (np.zeros(10, np.float32), np.zeros(17, np.complex128))):
        with pytest.raises(TypeError):
            fir_real.fir(x, h)
    with pytest.raises(ValueError):
        fir_real.fir(np.zeros(10, np.float32), np.zeros(17, np.float32), mode="xcorr")
    with pytest.raises(ValueError):
        fir_real.fir(np.zeros((2, 2, 10), np.float32), np.zeros(17, np.float32))


def test_default_fft_size_rule():
    """fft_size=None: N = clamp(next_pow2(4 M), 256, 4096), the rule of smfft_amd.fir_fft_size; M >= 4096, an unsupported N and
    M >= N are refused before anything touches a device"""
    import smfft_amd
    from smfft_amd import fir_real
    for m in (1, 17, 64, 65, 128, 129, 257, 1024, 1025, 4095):
        assert fir_real.fir_fft_size(m) == smfft_amd.fir_fft_size(m) == frm.fft_size(m), m
    for m, n in ((1, 256), (65, 512), (257, 2048), (4095, 4096)):
        assert fir_real.fir_fft_size(m) == n
    for m in (0, 4096, 5000):
        with pytest.raises(ValueError):
            fir_real.fir_fft_size(m)
    with pytest.raises(ValueError):
        fir_real.fir(np.zeros(10, np.float32), np.zeros(4096, np.float32))
    with pytest.raises(ValueError):
        fir_real.fir(np.zeros(10, np.float32), np.zeros(17, np.float32), fft_size=8192)
    with pytest.raises(ValueError):
        fir_real.fir(np.zeros(10, np.float32), np.zeros(256, np.float32), fft_size=256)


def test_import_does_not_load_the_library():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import smfft_amd, smfft_amd.fir_real as l; assert l._lib is None; "
            "maps = open('/proc/self/maps').read(); assert 'libsmfft_fir_real' not in maps; print('ok')")
    p = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout + p.stderr

"""The overlap-save FIR filter banks (smfft_amd/csrc/smfft_fir.hip, smfft_fir.hpp) on the CPU: the fp64 model of the segmentation
(tools/fir_plan_model.py) is np.convolve / np.correlate, the header's FirWindow compiled for the host gives the model's segment counts,
load starts, store windows and output indices, the gfx950 code of the new kernels keeps the library's rules (no scratch, no v_sin/v_cos,
no packed f32, the 16 signal loads of a segment back to back), and the C ABI declares, exports and validates the new entry points
without a device.  No GPU code is run (hipcc cross-compiles gfx950)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fir_plan_model as fm  # noqa: E402

from tests import addon_checks as ac  # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"
# the Makefile's HIPFLAGS for smfft_fir.o (less -fPIC / -Wall, which change no device code)
FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fno-slp-vectorize", "-I" + os.path.join(ROOT, "include")]
FIR_SRC = os.path.join(ROOT, "smfft_amd", "csrc", "smfft_fir.hip")
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


_taps_cases, _length_cases = ac.fir_taps_cases, ac.fir_length_cases


def _grid():
    for n in (256, 1024, 4096):
        for m in _taps_cases(n):
            for length in _length_cases(n, m):
                yield n, m, length


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("n", [256, 1024, 4096])
@pytest.mark.parametrize("correlate", [False, True])
def test_model_is_numpys_convolution_and_correlation(n, correlate):
    rng = np.random.default_rng(n + correlate)
    for m in _taps_cases(n):
        h = rng.standard_normal((2, m)) + 1j * rng.standard_normal((2, m))
        for length in _length_cases(n, m):
            x = rng.standard_normal((2, length)) + 1j * rng.standard_normal((2, length))
            want = fm.direct(x, h, correlate)
            got = fm.overlap_save(x, h, n, correlate)
            scale = max(np.max(np.abs(want)), 1e-300)
            assert np.max(np.abs(got - want)) <= 1e-12 * scale, (n, m, length, correlate)


def test_model_windows_tile_the_output_once():
    for n, m, length in _grid():
        for corr in (False, True):
            w = fm.Window(length, n, m, corr)
            assert w.segments() == -(-length // (n - m + 1))
            covered = np.zeros(length, np.int64)
            for s in range(w.segments()):
                b, e = w.store_window(s)
                assert b == m - 1 and b < e <= n, (n, m, length, s)
                # every output reads only the segment's own samples: x[n - m'] (convolve) / x[n + m'] (correlate), m' < M
                a = w.load_start(s)
                n0, n1 = w.output_index(s, b), w.output_index(s, e - 1)
                lo, hi = (n0 - (m - 1), n1) if not corr else (n0, n1 + m - 1)
                assert a <= lo and hi < a + n, (n, m, length, s, corr)
                covered[n0:n1 + 1] += 1
            assert np.all(covered == 1), (n, m, length, corr)


# ------------------------------------------------------------------------------------------------ header == model
@needs_hipcc
def test_header_window_is_the_models(tmp_path):
    cases = [(n, m, length) for n, m, length in _grid()] + [(1024, 257, (1 << 25) + 1000), (4096, 1025, (1 << 34) + 3)]
    src = tmp_path / "fir_window.hip"
    src.write_text(r'''
#include <cstdio>
#include "smfft_fir.hpp"
int main(int argc, char**) {
    int n, m, corr; long long L;
    while (argc == 1 && scanf("%d %d %lld %d", &n, &m, &L, &corr) == 4) {
        const smfft::FirWindow w{L, n, m, corr};
        const long long S = w.segments();
        printf("S %lld\n", S);
        const long long probe[6] = {0, 1, 2, S / 2, S - 2, S - 1};
        for (long long s : probe) {
            if (s < 0 || s >= S) continue;
            printf("%lld %lld %d %d %lld %lld\n", s, w.load_start(s), w.store_begin(), w.store_end(s), w.output_index(s, w.store_begin()),
                   w.output_index(s, w.store_end(s) - 1));
        }
    }
    long long tiles; int K, target;
    while (scanf("%lld %d %d", &tiles, &K, &target) == 3) printf("G %d\n", smfft::fir_filter_group_size(tiles, K, target));
    return 0;
}
''')
    exe = tmp_path / "fir_window"
    subprocess.check_call([HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "smfft_amd", "csrc"), str(src), "-o", str(exe)],
                          stderr=subprocess.DEVNULL)
    groups = [(tiles, k, 2048) for tiles in (1, 3, 20, 100, 2047, 2048, 5462, 1 << 40) for k in (1, 5, 32, 64, 200, 5000)]
    stdin = "".join(f"{n} {m} {length} {corr}\n" for n, m, length in cases for corr in (0, 1))
    out = subprocess.run([str(exe)], input=stdin, capture_output=True, text=True, check=True).stdout.split("\n")
    want = []
    for n, m, length in cases:
        for corr in (0, 1):
            w = fm.Window(length, n, m, corr)
            S = w.segments()
            want.append(f"S {S}")
            for s in (0, 1, 2, S // 2, S - 2, S - 1):
                if 0 <= s < S:
                    b, e = w.store_window(s)
                    want.append(f"{s} {w.load_start(s)} {b} {e} {w.output_index(s, b)} {w.output_index(s, e - 1)}")
    assert [line for line in out if line] == want
    gout = subprocess.run([str(exe), "groups"], input="".join(f"{t} {k} {g}\n" for t, k, g in groups), capture_output=True, text=True, check=True).stdout.split()
    gwant = []
    for tiles, k, target in groups:
        ngroups = min(k, max(1, -(-target // tiles)))
        gwant += ["G", str(-(-k // ngroups))]
    assert gout == gwant


# ------------------------------------------------------------------------------------------------ gfx950 code
@pytest.fixture(scope="module")
def isa():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = f"/tmp/smfft_test_fir_{os.getpid()}.s"
    p = subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", FIR_SRC, "-o", out], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    text = open(out).read()
    os.remove(out)
    return text


def _kernels(isa, frag):
    found = {}
    for m in re.finditer(r"^(_Z\w*%s\w*):[^\n]*\n(.*?)\n\s*s_endpgm" % frag, isa, re.S | re.M):
        found[m.group(1)] = [line.strip() for line in m.group(2).split("\n")]
    return found


def test_fir_kernels_have_no_scratch_no_transcendentals_no_packed_f32(isa):
    kernels = {**_kernels(isa, "fir_overlap_save_kernel"), **_kernels(isa, "fir_prepare_kernel")}
    assert len(kernels) == 10, sorted(kernels)
    for name, body in kernels.items():
        assert not [line for line in body if line.startswith("scratch_")], name
        assert not [line for line in body if re.match(r"v_(sin|cos)_", line)], name
        assert not [line for line in body if re.match(r"v_pk_\w+_f32", line)], name
        d = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(name), isa, re.S)
        assert d, name
        seg = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", d.group(1))
        assert seg and int(seg.group(1)) == 0, (name, seg and seg.group(1))


def test_fir_signal_loads_are_issued_back_to_back(isa):
    """the 16 signal loads of a segment (the kernel's only non-temporal loads) go out with no branch and no vmcnt(0) wait between the
    first and the last: no per-element "load or zero" (smfft_kernels.hpp, wave_chunk_to_lds)"""
    kernels = _kernels(isa, "fir_overlap_save_kernel")
    assert len(kernels) == 5
    for name, body in kernels.items():
        loads = [i for i, line in enumerate(body) if line.startswith("global_load") and re.search(r"\bnt\b", line)]
        assert len(loads) == 16, (name, len(loads))
        between = body[loads[0]:loads[-1] + 1]
        assert not [line for line in between if line.startswith(("s_cbranch", "s_branch", "s_setpc", "s_barrier"))], name
        assert not [line for line in between if re.search(r"vmcnt\(0\)", line)], name


# ------------------------------------------------------------------------------------------------ C ABI
DECLS = (
    "int smfft_fir_prepare(const void* d_taps, int n_taps, int n_filters, int FFT_size, int correlate, void* d_spectra, void* hip_stream);",
    "int smfft_fir_launch(const void* d_signal, long long signal_length, int n_channels, const void* d_spectra, int n_filters, int n_taps,\n"
    "                     int FFT_size, int correlate, void* d_output, void* hip_stream);",
    "int smfft_fir_benchmark(const void* d_signal, long long signal_length, int n_channels, const void* d_spectra, int n_filters, int n_taps,\n"
    "                        int FFT_size, int correlate, void* d_output, double* FFT_time);",
)
NAMES = ac.fir_names("smfft_fir")


def test_fir_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "smfft.h")).read()
    assert "FIR filter banks (overlap-save" in header
    for decl in DECLS:
        assert decl in header, decl
    import smfft_amd
    for name in NAMES:
        assert name in smfft_amd.api.EXPORTED_C_SYMBOLS
        assert getattr(smfft_amd.lib, name)
    assert callable(smfft_amd.fir) and callable(smfft_amd.fir_prepare) and callable(smfft_amd.fir_launch)
    nm = subprocess.run(["nm", "-D", "--defined-only", smfft_amd.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r" T %s$" % name, nm, re.M), name


def test_unsupported_combinations_return_minus_one_without_a_device():
    """all validation happens before any HIP call: these return -1 (or 0 for an empty signal) with no device and null pointers"""
    import smfft_amd
    ac.check_fir_rejections(smfft_amd.LIB_PATH, "smfft_fir", (256, 512, 1024, 2048, 4096))
    ac.check_fir_wrappers_refuse(smfft_amd.fir_prepare, smfft_amd.fir_launch, (256, 4096))


def test_default_fft_size_rule():
    """fft_size=None: N = clamp(next_pow2(4 M), 256, 4096); M >= 4096 is refused before anything touches a device"""
    import smfft_amd
    for m, n in ((1, 256), (17, 256), (64, 256), (65, 512), (257, 2048), (1024, 4096), (1025, 4096), (4095, 4096)):
        assert smfft_amd.fir_fft_size(m) == n, m
    for m in (0, 4096, 5000):
        with pytest.raises(ValueError):
            smfft_amd.fir_fft_size(m)
    with pytest.raises(ValueError):
        smfft_amd.fir(np.zeros(10, np.complex64), np.zeros(4096, np.complex64))

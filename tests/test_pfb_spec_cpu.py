"""Integrated power spectra of the polyphase filter banks (smfft_amd/csrc/smfft_pfb_spec.hip, smfft_pfb_spec.hpp,
include/smfft_pfb_spec.h) on the CPU: the header's PfbSpecPlan compiled for the host gives the model's spectra, groups, tiles and
offsets; the replay of the kernel's loop stores every output once and loads inside its own stream's window of (I T + P - 1) frames;
the gfx950 code of both accumulator forms keeps the library's rules (ten kernels, no scratch, no v_sin / v_cos, no packed f32) and
holds the VGPR and LDS figures the persistent grid rests on; the C ABI declares, exports and validates without a device; every
shipped kernel is in tests/pfb_spec_inventory.py with its tests.  No GPU code is run (hipcc cross-compiles gfx950)."""
import concurrent.futures
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pfb_model as pm  # noqa: E402
import pfb_real_model as prm  # noqa: E402
import pfb_spec_model as psm  # noqa: E402

from tests import addon_checks as ac  # noqa: E402
from tests import pfb_spec_inventory as sinv  # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "smfft_amd", "csrc")
SOURCE = os.path.join(CSRC, "smfft_pfb_spec.hip")
SIZES = (256, 512, 1024, 2048, 4096)
FFT_LDS = 4096 // 16 * 17 * 8            # the engine's region of 4096 points: 34816 B
ACC_LDS = 16 * 256 * 4                   # sixteen floats of 256 threads: 16384 B
VGPRS_PER_SIMD = 512
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


# ------------------------------------------------------------------------------------------------ the model
def test_model_is_the_banks_power_summed_over_frames():
    rng = np.random.default_rng(0)
    N = 256
    for real in (False, True):
        chunk = 2 * N if real else N
        for P, C, T, frames, tail in ((1, 1, 1, 3, 0), (3, 2, 4, 10, 6), (4, 3, 5, 15, 100), (2, 1, 7, 6, 0)):
            L = (frames + P - 1) * chunk + tail
            x = rng.standard_normal((C, L)) if real else rng.standard_normal((C, L)) + 1j * rng.standard_normal((C, L))
            h = rng.standard_normal(P * chunk)
            S, m = psm.integrate(x, h, N, T, real)
            n = frames // T
            assert psm.spectra(L, N, P, T, real) == n and S.shape == (C, n, N) and m.shape == (C, n)
            p = prm.power(prm.pfb_real(x, h, N)) if real else pm.pfb(x, h, N, power=True)
            for i in range(n):
                assert np.allclose(S[:, i], p[:, i * T:(i + 1) * T].sum(axis=1), rtol=1e-13)
                assert np.allclose(m[:, i], p[:, i * T:(i + 1) * T].max(axis=-1).sum(axis=1), rtol=1e-13)
            assert np.all(m >= S.max(axis=-1) * (1 - 1e-13))


# ------------------------------------------------------------------------------------------------ header == model
def _plan_cases():
    cases = []
    for N in SIZES:
        per = 4096 // N
        for P in (1, 4, 32):
            for T in (1, 3, 64):
                for frames in (0, 1, T - 1, T, T + 1, (per + 1) * T + T // 2, (2 * per + 1) * T):
                    for C in (1, 3):
                        cases.append(((frames + P - 1) * N + N // 2 if frames else P * N - 1, N, P, C, T))
    # C L beyond 2^32, offsets beyond 2^31
    cases += [((1 << 31) + 12345, 1024, 4, 2, 64), ((1 << 33) + 7, 4096, 16, 3, 5), ((1 << 32) + 255, 256, 32, 5, 1000)]
    return cases


@needs_hipcc
def test_header_plan_is_the_models(tmp_path):
    src = tmp_path / "pfb_spec_plan.hip"
    src.write_text(r'''
#include <cstdio>
#include "smfft_pfb_spec.hpp"
int main() {
    long long L; int N, P, C, T;
    while (scanf("%lld %d %d %d %d", &L, &N, &P, &C, &T) == 5) {
        const smfft::PfbSpecPlan w{L, N, P, C, T};
        const long long groups = w.groups(), tiles = w.tiles();
        printf("I %lld %lld %lld %d %lld %lld\n", w.frames(), w.spectra(), groups, w.per_tile(), tiles, w.used());
        const long long probe[7] = {0, 1, w.spectra() - 1, w.spectra(), groups / 2, groups - 2, groups - 1};
        for (long long g : probe) {
            if (g < 0 || g >= groups) continue;
            printf("%lld %lld %lld %lld %lld %lld\n", g, w.stream_of(g), w.spectrum_of(g), w.input_offset(g, 0), w.input_offset(g, T - 1), w.output_offset(g));
        }
        if (tiles > 0) {
            printf("T");
            for (int j = 0; j < w.per_tile(); ++j) printf(" %lld", w.group_of(tiles - 1, j));
            printf(" G %lld %lld %lld\n", w.grid(1), w.grid(tiles), w.grid(768));
        }
    }
    return 0;
}
''')
    exe = tmp_path / "pfb_spec_plan"
    subprocess.check_call([HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I" + CSRC, str(src), "-o", str(exe)], stderr=subprocess.DEVNULL)
    cases = _plan_cases()
    out = subprocess.run([str(exe)], input="".join("%d %d %d %d %d\n" % c for c in cases), capture_output=True, text=True, check=True).stdout.split("\n")
    want = []
    for L, N, P, C, T in cases:
        w = psm.Plan(L, N, P, C, T)
        F, n, groups, tiles = w.frames(), w.spectra(), w.groups(), w.tiles()
        assert F == max(L // N - P + 1, 0) and n == F // T and groups == C * n and tiles == -(-groups // (4096 // N))
        want.append(f"I {F} {n} {groups} {w.per_tile()} {tiles} {w.used()}")
        for g in (0, 1, n - 1, n, groups // 2, groups - 2, groups - 1):
            if 0 <= g < groups:
                want.append(f"{g} {w.stream_of(g)} {w.spectrum_of(g)} {w.input_offset(g, 0)} {w.input_offset(g, T - 1)} {w.output_offset(g)}")
                # the group's last frame ends inside what its stream reads, and that inside the stream
                assert w.input_offset(g, T - 1) + P * N <= w.stream_of(g) * L + w.used() <= (w.stream_of(g) + 1) * L
        if tiles:
            want.append("T " + " ".join(str(w.group_of(tiles - 1, j)) for j in range(w.per_tile())) + f" G {w.grid(1)} {w.grid(tiles)} {w.grid(768)}")
    assert [line for line in out if line] == want
    # the cases the issue names are in the grid
    plans = [psm.Plan(*c) for c in cases]
    assert any(w.frames() % w.T for w in plans if w.spectra()), "F not a multiple of T"
    assert any(w.spectra() == 0 and w.frames() > 0 for w in plans) and any(w.frames() == 0 for w in plans), "I = 0"
    assert any(w.C == 3 and w.spectra() % w.per_tile() for w in plans if w.per_tile() > 1), "tiles straddling streams"
    assert any(w.input_offset(w.groups() - 1, w.T - 1) > 1 << 32 for w in plans if w.groups())


# ------------------------------------------------------------------------------------------------ the replay
@pytest.mark.parametrize("case", [(9 * 256 + 100, 256, 4, 3, 2), (20 * 256, 256, 2, 5, 1), (5 * 512, 512, 1, 1, 5), (14 * 1024 + 1023, 1024, 8, 3, 3),
                                  (40 * 2048, 2048, 32, 2, 4), (9 * 4096 + 5, 4096, 2, 3, 3), (3 * 4096, 4096, 4, 2, 1), (6 * 1024, 1024, 4, 2, 4)])
def test_replay_stores_once_and_loads_inside_the_window(case):
    L, N, P, C, T = case
    w = psm.Plan(L, N, P, C, T)
    n = w.spectra()
    if n == 0:
        assert w.tiles() == 0 and w.used() == 0
        return
    used = (n * T + P - 1) * N
    assert w.used() == used <= L
    for G in (1, 3, w.tiles() + 4):
        loads, stores, taps = psm.replay(w, w.grid(G))
        assert np.array_equal(np.sort(stores), np.arange(C * n * N)), "every output element exactly once"
        assert taps == P * N - 1
        seen = set()
        for group, c, t, addr in loads:
            assert addr.shape == (P, N)
            assert addr.min() >= c * L and addr.max() < c * L + used, (case, group, t)
            if group >= 0:
                f = (group - c * n) * T + t
                assert np.array_equal(np.sort(addr, axis=1), c * L + (f + np.arange(P))[:, None] * N + np.arange(N)[None, :])
                seen.add((c, f))
        assert seen == {(c, f) for c in range(C) for f in range(n * T)}, "every frame below I T, and none beyond"


# ------------------------------------------------------------------------------------------------ gfx950 code
def _shipped_form():
    """the accumulator form the Makefile builds: PFB_SPEC_ACC_LDS is empty there, so it is the source's default"""
    assert re.search(r"^PFB_SPEC_ACC_LDS \?=\s*$", open(os.path.join(CSRC, "Makefile")).read(), re.M)
    m = re.search(r"#ifndef SMFFT_PFB_SPEC_ACC_LDS\n#define SMFFT_PFB_SPEC_ACC_LDS ([01])\n#endif", open(SOURCE).read())
    assert m
    return int(m.group(1))


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """{accumulator form: {N: assembly}}: the shipped form as the Makefile compiles it (no define), the other one with its define"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    tmp = tmp_path_factory.mktemp("pfb_spec_isa")
    shipped = _shipped_form()

    def compile_one(job):
        form, n = job
        define = [] if form == shipped else [f"-DSMFFT_PFB_SPEC_ACC_LDS={form}"]
        return ac.device_asm(SOURCE, ["-I" + CSRC] + ac.makefile_flags("PFB_SPEC", n) + define + [f"-DSMFFT_PFB_SPEC_N={n}"], tmp / f"spec_{form}_{n}.s")
    jobs = [(form, n) for form in (shipped, 1 - shipped) for n in SIZES]
    with concurrent.futures.ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
        texts = list(pool.map(compile_one, jobs))
    out = {0: {}, 1: {}}
    for (form, n), text in zip(jobs, texts):
        out[form][n] = text
    return out


def _workgroups_per_cu(vgprs, lds):
    """what a compute unit holds of a 256-thread workgroup (one wave per SIMD): by its registers (granules of 8) and by its LDS"""
    return min(VGPRS_PER_SIMD // (-(-vgprs // 8) * 8), ac.LDS_PER_CU // lds)


def _figures(isa, form):
    """{(kernel, N): (VGPRs, LDS bytes)} after the rules every kernel of the form keeps"""
    out = {}
    for n, text in isa[form].items():
        descs = ac.descriptors(text)
        assert len(descs) == 2, (form, n, sorted(descs))                   # one kernel per bank, nothing else
        for kernel in ("pfb_spec_kernel", "pfb_real_spec_kernel"):
            found = ac.pfb_kernels(text, kernel)
            assert len(found) == 1, (form, n, kernel, sorted(found))
            (name, body), = found.items()
            assert "%sILi%dE" % (kernel, n) in name and name in descs
            assert not [line for line in body if line.startswith("scratch_")], name
            assert not [line for line in body if re.match(r"v_(sin|cos)_", line)], name
            assert not [line for line in body if re.match(r"v_pk_\w+_f32", line)], name
            assert ac.descriptor_field(descs, name, "private_segment_fixed_size") == 0, name
            # the signal loads are plain, the shipped policy (profiles/r15_pfb_spec_ab.txt); the sums go out in sixteen non-temporal stores
            assert not [line for line in body if line.startswith("global_load") and line.endswith(" nt")], name
            assert len([line for line in body if line.startswith("global_store")]) == 16, name
            assert all(line.endswith(" nt") for line in body if line.startswith("global_store")), name
            out[(kernel, n)] = (ac.descriptor_field(descs, name, "next_free_vgpr"), ac.descriptor_field(descs, name, "group_segment_fixed_size"))
    assert len(out) == 10
    return out


def test_lds_form_fits_three_workgroups_per_cu_without_scratch(isa):
    """sums in LDS: 34816 + 16384 = 51200 B per workgroup, three of them in a compute unit's 160 KiB, and at most 168 VGPRs at every
    length in both banks: three waves per SIMD"""
    for (kernel, n), (vgprs, lds) in _figures(isa, 1).items():
        print(f"LDS form  {kernel:22s} N={n:5d}: {vgprs} VGPRs, {lds} B of LDS -> {_workgroups_per_cu(vgprs, lds)} workgroups per compute unit")
        assert lds == FFT_LDS + ACC_LDS == 51200 and 3 * lds <= ac.LDS_PER_CU, (kernel, n, lds)
        assert vgprs <= ac.PFB_VGPR_BUDGET, (kernel, n, vgprs)
        assert _workgroups_per_cu(vgprs, lds) == 3


def test_register_form_has_no_scratch_and_at_least_two_workgroups_per_cu(isa):
    """sums in registers: the engine's LDS alone, and whatever occupancy the sixteen extra registers leave -- two or three workgroups per
    compute unit, never one"""
    for (kernel, n), (vgprs, lds) in _figures(isa, 0).items():
        print(f"reg form  {kernel:22s} N={n:5d}: {vgprs} VGPRs, {lds} B of LDS -> {_workgroups_per_cu(vgprs, lds)} workgroups per compute unit")
        assert FFT_LDS <= lds <= FFT_LDS + 16, (kernel, n, lds)
        assert vgprs <= 256 and _workgroups_per_cu(vgprs, lds) in (2, 3), (kernel, n, vgprs)


def test_shipped_objects_are_one_of_the_two_forms_and_the_grid_asks_the_device(isa):
    """ten kernels as the Makefile builds them; the launcher sizes the grid by the occupancy the runtime reports for the compiled kernel
    (its VGPRs and LDS, the figures above), not by a constant"""
    figures = _figures(isa, _shipped_form())
    assert len(figures) == 10
    source = open(SOURCE).read()
    assert "hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, kPfbThreads, 0)" in source and "kWorkgroupsPerCu" not in source


def test_the_sum_keeps_both_roundings(isa):
    """the source hands every power value through an empty asm before it is added (the body says why), and in the code of both forms and
    banks the sixteen power values of a frame are followed by sixteen plain v_add_f32, the sums' own additions.  That the bits
    are the definition's is the GPU test's to show (check_output_is_the_shipped_power_mode_summed_in_frame_order of tests/test_pfb_spec_gpu.py)"""
    assert 'asm volatile("" : "+v"(p));' in open(SOURCE).read()
    for form in (0, 1):
        for n, text in isa[form].items():
            for kernel in ("pfb_spec_kernel", "pfb_real_spec_kernel"):
                (name, body), = ac.pfb_kernels(text, kernel).items()
                marks = [i for i, line in enumerate(body) if line.startswith(";;#ASMSTART")]
                assert len(marks) >= 16, (name, len(marks))          # (the real bank's split through LDS has one of its own before them)
                adds, span = 0, []                          # from the first of the last sixteen markers to the sixteenth add
                for line in body[marks[-16]:]:
                    span.append(line)
                    adds += line.startswith("v_add_f32")
                    if adds == 16:
                        break
                assert adds == 16, (name, adds)


# ------------------------------------------------------------------------------------------------ C ABI
@pytest.fixture(scope="module")
def ps():
    from smfft_amd import pfb_spec
    pfb_spec.lib()
    return pfb_spec


def _names():
    return sorted(f"{prefix}_{f}" for prefix in ("smfft_pfb_spec", "smfft_pfb_real_spec") for f in ("spectra", "launch", "benchmark", "launch_tuned"))


def test_header_declarations_equal_the_ctypes_signatures(ps):
    header = open(os.path.join(ROOT, "include", "smfft_pfb_spec.h")).read()
    for phrase in ("Out of scope", "N >= 8192", "cross-products between streams", "C*I*N/4096 workgroups", "sums the few resulting spectra afterwards",
                   "growth of fp32 rounding with T", "exactly once", "no atomics"):
        assert phrase in header, phrase
    decl = ac.declarations("smfft_pfb_spec.h")
    assert sorted(decl) == sorted(ps.SIGS) == _names() and len(decl) == 8
    for name, (res, args) in decl.items():
        assert ps.SIGS[name] == ac.signature(res, args), name
    for prefix in ps.PREFIXES:
        # launch_tuned = the arguments of launch + max_workgroups; benchmark = launch with the timer in the stream's place
        assert ps.SIGS[prefix + "_launch_tuned"][1] == ps.SIGS[prefix + "_launch"][1] + [ctypes.c_int]
        assert ps.SIGS[prefix + "_benchmark"][1][:-1] == ps.SIGS[prefix + "_launch"][1][:-1]
    # the real bank's functions are the complex bank's, one for one
    for name in ps.SIGS:
        assert ps.SIGS[name] == ps.SIGS[name.replace("pfb_real_spec", "pfb_spec")], name
    assert tuple(ps.SIZES) == SIZES


def test_library_exports_exactly_the_eight_symbols(ps):
    nm = subprocess.run(["nm", "-D", "--defined-only", ps.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r" T (smfft_\w+)$", nm, re.M)) == _names()
    # and the banks' libraries keep their lists: nothing of the spectra went into them
    from smfft_amd import pfb, pfb_real
    for bank in (pfb, pfb_real):
        nm = subprocess.run(["nm", "-D", "--defined-only", bank.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert not re.findall(r"spec", nm), bank.LIB_PATH


def test_unsupported_combinations_return_minus_one_without_a_device(ps):
    """all validation happens before any HIP call: these return -1 (or 0 when there is no whole integration) with null pointers"""
    lib = ps.lib()
    t = ctypes.c_double(0.0)
    for real, prefix in enumerate(ps.PREFIXES):
        spectra, launch, benchmark, launch_tuned = (getattr(lib, f"{prefix}_{f}") for f in ("spectra", "launch", "benchmark", "launch_tuned"))
        unit = 2 if real else 1
        bad = [(1 << 20, 1, n, 4, 8) for n in (0, 128, 1000, 8192, 16384, -1024)] + [(1 << 20, 1, 1024, p, 8) for p in (0, 33, -1)]
        bad += [(1 << 20, 1, 1024, 4, T) for T in (0, -1, -64)] + [(1 << 20, c, 1024, 4, 8) for c in (0, -1)] + [(-2, 1, 1024, 4, 8), (-1, 1, 1024, 4, 8)]
        if real:
            bad += [((1 << 20) + 1, 1, 1024, 4, 8), (1, 1, 256, 1, 1), (8 * 2048 + 1, 2, 1024, 4, 1)]       # odd
        for L, C, N, P, T in bad:
            assert launch(None, L, C, None, N, P, T, None, None) == -1, (prefix, L, C, N, P, T)
            assert launch_tuned(None, L, C, None, N, P, T, None, None, 3) == -1, (prefix, L, C, N, P, T)
            assert benchmark(None, L, C, None, N, P, T, None, ctypes.byref(t)) == -1, (prefix, L, C, N, P, T)
            if C > 0:
                assert spectra(L, N, P, T) == -1, (prefix, L, N, P, T)
        assert launch_tuned(None, 1 << 20, 1, None, 1024, 4, 8, None, None, -1) == -1
        # no whole integration is not an error: nothing is launched.  No frame; fewer frames than T
        for L, T in ((0, 1), (unit * 1023, 1), (unit * (4 * 1024 - 1), 1), (unit * (4 + 6) * 1024, 8), (unit * 4 * 1024, 2)):
            assert spectra(L, 1024, 4, T) == 0, (prefix, L, T)
            assert launch(None, L, 2, None, 1024, 4, T, None, None) == 0
            assert launch_tuned(None, L, 2, None, 1024, 4, T, None, None, 7) == 0
            assert benchmark(None, L, 2, None, 1024, 4, T, None, ctypes.byref(t)) == 0
    assert t.value == 0.0
    with pytest.raises(ValueError):
        ps.spectra(1000, 100, 4, 2)
    with pytest.raises(ValueError):
        ps.spectra(1 << 20, 1024, 4, 0)
    with pytest.raises(ValueError):
        ps.spectra(8 * 2048 + 1, 1024, 4, 2, real=True)
    with pytest.raises(RuntimeError):
        ps.launch(None, 1 << 20, 1, None, 8192, 4, 8, None)
    with pytest.raises(RuntimeError):
        ps.launch_tuned(None, 1 << 20, 1, None, 1024, 4, 8, None, -1, real=True)
    with pytest.raises(ValueError):
        ps.integrate(np.zeros(4096, np.complex64), np.zeros(100, np.float32), 256, 2)
    with pytest.raises(ValueError):
        ps.integrate(np.zeros(4096, np.complex64), np.zeros(512, np.float32), 256, 2, real=True)
    assert ps.integrate(np.zeros((2, 1000), np.complex64), np.zeros(1024, np.float32), 256, 2).shape == (2, 0, 256)
    assert ps.integrate(np.zeros((2, 1000), np.float32), np.zeros(1024, np.float32), 256, 2, real=True).shape == (2, 0, 256)


def test_spectra_over_ragged_lengths_and_prototype(ps):
    from smfft_amd import pfb, pfb_real
    for N in SIZES:
        for P in (1, 4, 32):
            for T in (1, 3, 64):
                for frames in (0, 1, T - 1, T, 2 * T + 1, 1000):
                    for real, bank in ((False, pfb), (True, pfb_real)):
                        L = ((frames + P - 1) * N + N - 1) * (2 if real else 1) if frames else 0
                        assert ps.spectra(L, N, P, T, real=real) == bank.frames(L, N, P) // T == psm.spectra(L, N, P, T, real) == frames // T
    assert ps.spectra((1 << 34) + 6, 1024, 4, 64, real=True) == (((1 << 34) + 6) // 2048 - 3) // 64
    assert np.array_equal(ps.prototype(512, 3), pfb.prototype(512, 3)) and np.array_equal(ps.prototype(512, 3, real=True), pfb_real.prototype(512, 3))
    assert np.array_equal(ps.prototype(256, 2, "blackman", real=True), pfb_real.prototype(256, 2, "blackman"))


def test_every_kernel_is_in_the_inventory_with_its_tests(ps):
    """the rule of tests/test_kernel_inventory.py, without the "host" kind (tests/pfb_spec_inventory.py says why)"""
    ac.check_inventory(ps.LIB_PATH, sinv.KERNELS, "smfft_pfb_", 10, kinds=("tests", "bounds", "probes"))

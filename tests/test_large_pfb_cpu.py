"""The polyphase filter bank channelizer for N = 8192 / 16384 channels (include/smfft/smfft_large_pfb.hpp, smfft_amd/csrc/smfft_large_pfb.hip,
include/smfft_large_pfb.h) on the CPU: the fp64 model's two forms of the definition agree, the header's LargePfbSchedule and PfbPlan
compiled for the host give the model's grids, pairs and offsets, both schedules produce every pair exactly once, the replay of the
kernel's loops stores every output once and loads inside its own stream's window, the gfx950 code keeps the library's rules (at most
128 VGPRs, no scratch, the engine's LDS image, no v_sin / v_cos, no packed f32, the sixteen signal loads of a tap together), the C ABI
declares, exports and validates without a device, every shipped kernel is in tests/large_pfb_inventory.py with its tests, and the
leakage figures the GPU test relies on hold for the model.  No GPU code is run (hipcc cross-compiles gfx950)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import large_pfb_model as lpm  # noqa: E402

from tests import addon_checks as ac  # noqa: E402
from tests import large_pfb_inventory as linv  # noqa: E402

HIPCC = ac.HIPCC
CSRC = ac.CSRC
SIZES = (8192, 16384)
STEM = "smfft_large_pfb"
NAMES = tuple(f"{STEM}_{f}" for f in ("frames", "launch", "benchmark", "launch_tuned", "default_schedule"))
LDS_BYTES = {8192: 16 * (512 + 2) * 8, 16384: 16 * (1024 + 2) * 8}      # LargeGeometry<N>::kLdsBytes
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def _rand(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# ------------------------------------------------------------------------------------------------ the model
def test_models_two_forms_agree():
    """the weighted frames + FFT against the direct sum: whole spectra at a small N (the definition is the same at every N), sampled
    channels at the two lengths of this bank"""
    rng = np.random.default_rng(0)
    for P, C, L in ((1, 1, 256), (3, 2, 6 * 256 + 17), (32, 1, 34 * 256 + 3)):
        x, h = _rand(rng, (C, L)), rng.standard_normal(P * 256)
        a, b = lpm.pfb(x, h, 256), lpm.pfb_direct(x, h, 256)
        assert a.shape == (C, L // 256 - P + 1, 256)
        assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b)), (P, C, L)
    for N in SIZES:
        P, F = 3, 2
        x, h = _rand(rng, (1, (F + P - 1) * N + 5)), rng.standard_normal(P * N)
        a = lpm.pfb(x, h, N)
        ks = np.array([0, 1, 100, N // 2, N - 1])
        m = np.arange(P * N)
        for f in range(F):
            E = np.exp(-2j * np.pi * ((ks[:, None] * m[None, :]) % N) / N)
            b = E @ (h * x[0, f * N:f * N + P * N])
            assert np.max(np.abs(a[0, f, ks] - b)) <= 1e-11 * np.max(np.abs(a[0, f])), (N, f)


@pytest.mark.parametrize("N", SIZES)
def test_model_with_one_tap_of_ones_is_the_plain_fft(N):
    rng = np.random.default_rng(N)
    x = _rand(rng, (2, 3 * N + 11))
    want = np.fft.fft(x[:, :3 * N].reshape(2, 3, N), axis=-1)
    assert np.max(np.abs(lpm.pfb(x, np.ones(N), N) - want)) <= 1e-12 * np.max(np.abs(want))


# ------------------------------------------------------------------------------------------------ header == model
GRIDS = (1, 7, 8, 20, 24, 512)


def _schedule_cases():
    """(L, N, P, C, cap, form)"""
    cases = []
    for N in SIZES:
        for P in (1, 32):
            for G in GRIDS:
                for form in (1, 2):
                    shapes = [(P * N - 1, 1), (P * N + 5, 3)]                                        # F = 0; F = 1, three streams
                    shapes += [((k * G + d + P - 1) * N + N // 2, 1) for k in (1, 3) for d in (-1, 0, 1)]   # pairs = k G - 1, k G, k G + 1, ragged L
                    shapes += [((G + 3 + P - 1) * N + 7, 3), ((5 + P - 1) * N, 2)]                   # pairs straddle streams; pairs < G for the large grids
                    cases += [(L, N, P, C, G, form) for L, C in shapes]
    # C F N and C L beyond 2^32
    cases += [((1 << 33) + 7, 16384, 16, 3, 512, form) for form in (1, 2)] + [((1 << 32) + 255, 8192, 32, 5, 256, form) for form in (1, 2)]
    cases += [((1 << 31) + 12345, 8192, 4, 2, 20, 2)]
    return cases


ENUMERATE = 6000      # launches of up to this many pairs are printed whole


@needs_hipcc
def test_header_schedule_is_the_models(tmp_path):
    src = tmp_path / "large_pfb_schedule.hip"
    src.write_text(r'''
#include <cstdio>
#include "smfft/smfft_large_pfb.hpp"
int main() {
    long long L, cap; int N, P, C, form;
    while (scanf("%lld %d %d %d %lld %d", &L, &N, &P, &C, &cap, &form) == 6) {
        const smfft::PfbPlan w{L, N, P, C};
        const long long pairs = w.pairs();
        printf("F %lld %lld\n", w.frames(), pairs);
        if (pairs == 0) continue;
        const smfft::large::LargePfbSchedule s = smfft::large::LargePfbSchedule::make(pairs, cap, form);
        const long long rounds = s.rounds();
        printf("S %d %d %lld\n", s.grid, s.form, rounds);
        if (pairs <= ''' + str(ENUMERATE) + r''') {
            for (int b = 0; b < s.grid; ++b) {
                printf("%d:", b);
                for (long long t = 0; t * s.grid < s.pairs; ++t) printf(" %lld", s.pair_of(b, t));
                printf("\n");
            }
        }
        const int bs[6] = {0, 1, 7, 8, s.grid / 2, s.grid - 1};
        const long long ts[4] = {0, 1, rounds / 2, rounds - 1};
        for (int b : bs)
            for (long long t : ts) {
                if (b >= s.grid || t >= rounds) continue;
                const long long g = s.pair_of(b, t);
                if (g < 0) { printf("%d %lld -1\n", b, t); continue; }
                printf("%d %lld %lld %lld %lld %lld %lld\n", b, t, g, w.stream_of(g), w.frame_of(g), w.input_offset(g), w.output_offset(g));
            }
    }
    return 0;
}
''')
    exe = tmp_path / "large_pfb_schedule"
    subprocess.check_call([HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                          stderr=subprocess.DEVNULL)
    cases = _schedule_cases()
    out = subprocess.run([str(exe)], input="".join("%d %d %d %d %d %d\n" % c for c in cases), capture_output=True, text=True, check=True).stdout.split("\n")
    want = []
    seen = {"F0": 0, "F1": 0, "below": 0, "ragged": 0, "straddle": 0, "fallback": 0, "rounded": 0, "big": 0}
    for L, N, P, C, cap, form in cases:
        w = lpm.Plan(L, N, P, C)
        F, pairs = w.frames(), w.pairs()
        assert F == max(L // N - P + 1, 0)
        want.append(f"F {F} {pairs}")
        seen["F0"] += F == 0 and L > 0
        if pairs == 0:
            continue
        s = lpm.Schedule.make(pairs, cap, form)
        assert s.grid == (min(pairs, cap) if s.form == 1 else min(pairs, cap) // 8 * 8) and 1 <= s.grid <= cap
        assert s.form == (2 if form == 2 and min(pairs, cap) >= 8 else 1)
        rounds = s.rounds()
        want.append(f"S {s.grid} {s.form} {rounds}")
        seen["F1"] += F == 1
        seen["below"] += pairs < cap
        seen["ragged"] += pairs % s.grid in (1, s.grid - 1) and pairs > s.grid
        seen["straddle"] += C > 1 and F % s.grid != 0 and pairs > s.grid
        seen["fallback"] += form == 2 and s.form == 1
        seen["rounded"] += s.form == 2 and s.grid < min(pairs, cap)
        seen["big"] += pairs * N > 1 << 32 and C * L > 1 << 32
        if pairs <= ENUMERATE:
            every = []
            for b in range(s.grid):
                mine = [s.pair_of(b, t) for t in range(rounds)]
                want.append(f"{b}:" + "".join(f" {g}" for g in mine))
                assert [g for g in mine if g >= 0] == s.pairs_of(b)
                every += s.pairs_of(b)
            assert sorted(every) == list(range(pairs)), ("every pair exactly once", L, N, P, C, cap, form)
        for b in (0, 1, 7, 8, s.grid // 2, s.grid - 1):
            for t in (0, 1, rounds // 2, rounds - 1):
                if b >= s.grid or t >= rounds:
                    continue
                g = s.pair_of(b, t)
                want.append(f"{b} {t} -1" if g < 0 else f"{b} {t} {g} {w.stream_of(g)} {w.frame_of(g)} {w.input_offset(g)} {w.output_offset(g)}")
    assert [line for line in out if line] == want
    # the cases the issue names are in the grid
    assert all(seen.values()), seen


def test_both_schedules_produce_every_pair_exactly_once():
    """each round's block of G consecutive pairs is permuted: within a round the slots of the G workgroups are 0 ... G - 1"""
    for G in (8, 16, 24, 512):
        s = lpm.Schedule(10 * G + 3, G, 2)
        assert sorted(s.slot(b) for b in range(G)) == list(range(G))
        # the workgroups b = i (mod 8) take G / 8 consecutive pairs of a round
        for i in range(8):
            assert [s.slot(b) for b in range(i, G, 8)] == list(range(i * (G // 8), (i + 1) * (G // 8)))
    for pairs in (1, 7, 8, 9, 23, 24, 25, 100, 511, 512, 513, 1537):
        for cap in GRIDS:
            for form in (1, 2):
                s = lpm.Schedule.make(pairs, cap, form)
                every = [g for b in range(s.grid) for g in s.pairs_of(b)]
                assert sorted(every) == list(range(pairs)), (pairs, cap, form)
                assert all(s.pairs_of(b) for b in range(s.grid)), "a workgroup of the grid without work"


# ------------------------------------------------------------------------------------------------ the replay
@pytest.mark.parametrize("case", [(7 * 8192 + 100, 8192, 4, 3, 7, 1), (5 * 8192, 8192, 1, 1, 8, 2), (12 * 8192 + 8191, 8192, 8, 3, 8, 2),
                                  (40 * 16384, 16384, 32, 2, 16, 2), (6 * 16384 + 5, 16384, 2, 3, 20, 2), (3 * 16384, 16384, 4, 2, 3, 1)])
def test_replay_stores_once_and_loads_inside_the_window(case):
    L, N, P, C, cap, form = case
    plan = lpm.Plan(L, N, P, C)
    if plan.pairs() == 0:
        assert plan.frames() == 0
        return
    assert lpm.check_replay(plan, lpm.Schedule.make(plan.pairs(), cap, form)) == plan.pairs()


# ------------------------------------------------------------------------------------------------ gfx950 code
@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """{N: gfx950 assembly of smfft_large_pfb_<N>.o as the Makefile compiles it: -I. and LARGE_PFB_FLAGS_<N>}"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    tmp = tmp_path_factory.mktemp("large_pfb_isa")
    return {n: ac.device_asm(os.path.join(CSRC, STEM + ".hip"), ["-I" + CSRC] + ac.makefile_flags("LARGE_PFB", n) + [f"-DSMFFT_LARGE_PFB_N={n}"],
                             tmp / f"{STEM}_{n}.s") for n in SIZES}


def test_kernels_keep_the_budgets_of_the_large_engine(isa):
    """two kernels per length and nothing else, four in all: at most 128 VGPRs (four waves per SIMD: two 8192 workgroups or one 16384
    workgroup per compute unit, the figure the launcher's grid rests on), no scratch, no private segment, the engine's LDS image, no
    v_sin / v_cos, no packed f32; the six barriers of one transform"""
    total = 0
    for n, text in isa.items():
        kernels, descs = ac.pfb_kernels(text, "pfb_large"), ac.descriptors(text)
        assert len(kernels) == 2 and len(descs) == 2, (n, sorted(kernels), sorted(descs))
        total += len(kernels)
        for name, body in kernels.items():
            assert "pfb_largeILi%dE" % n in name
            assert not [line for line in body if line.startswith("scratch_")], name
            assert not [line for line in body if re.match(r"v_(sin|cos)_", line)], name
            assert not [line for line in body if re.match(r"v_pk_\w+_f32", line)], name
            assert ac.descriptor_field(descs, name, "private_segment_fixed_size") == 0, name
            vgprs, lds = ac.descriptor_field(descs, name, "next_free_vgpr"), ac.descriptor_field(descs, name, "group_segment_fixed_size")
            print(f"N={n:5d} {'power  ' if f'ILi{n}ELi1E' in name else 'complex'}: {vgprs} VGPRs, {lds} B of LDS")
            assert lds == LDS_BYTES[n] and (ac.LDS_PER_CU // lds) == (2 if n == 8192 else 1), name
            assert vgprs <= 128, (name, vgprs)
            assert len([line for line in body if line.startswith("s_barrier")]) == 6, name
        assert not re.search(r"\bscratch_", text)
    assert total == 4


def test_signal_loads_of_a_tap_are_issued_together(isa):
    """the tap loop is the loop around the kernel's sched_barrier.  Before the barrier: the sixteen signal loads of a tap -- a scalar base
    and one 32-bit lane offset each, plain in the shipped build -- contiguous up to scalar address arithmetic, with no branch, barrier or
    vmcnt(0) among them.  Behind it, before the loop's backward branch: the sixteen coefficient loads, of the same form.  (The rule of
    addon_checks.check_pfb_signal_loads, which finds the signal loads of the small banks by their nt suffix.)"""
    signal = r"global_load_dwordx2 v\[\d+:\d+\], v\d+, s\[\d+:\d+\]( offset:-?\d+)?$"
    tap = r"global_load_dword v\d+, v\d+, s\[\d+:\d+\]( offset:-?\d+)?$"
    arithmetic = r"(s_add|s_addc|s_mov|s_nop|;)"
    for n, text in isa.items():
        for name, body in ac.pfb_kernels(text, "pfb_large").items():
            assert not [line for line in body if line.startswith("global_load") and line.endswith(" nt")], name     # the shipped policy
            fences = [i for i, line in enumerate(body) if line.startswith("; sched_barrier")]
            assert len(fences) == 1, (name, fences)
            fence = fences[0]
            top = max(i for i in range(fence) if re.match(r"\.LBB\d+_\d+:", body[i]))
            label = body[top].split(":")[0]
            end = next(i for i in range(fence, len(body)) if body[i].startswith("s_cbranch"))
            assert body[end].split()[-1] == label, (name, label, body[end])          # a loop: the branch goes back to the label
            loads = [i for i in range(top, fence) if re.match(signal, body[i])]
            assert len(loads) == 16 and not [i for i in range(top, fence) if body[i].startswith("global_load") and i not in loads], (name, len(loads))
            between = body[loads[0]:loads[-1] + 1]
            assert not [line for line in between if line.startswith(("s_cbranch", "s_branch", "s_setpc", "s_barrier"))], name
            assert not [line for line in between if re.search(r"vmcnt\(0\)", line)], name
            others = [line for line in between if line and not line.startswith("global_load_dwordx2")]
            assert all(re.match(arithmetic, line) for line in others), (name, others)
            taps = [i for i in range(fence, end) if re.match(tap, body[i])]
            assert len(taps) == 16 and not [i for i in range(fence, end) if body[i].startswith("global_load") and i not in taps], (name, len(taps))


# ------------------------------------------------------------------------------------------------ C ABI
@pytest.fixture(scope="module")
def large_pfb():
    from smfft_amd import large_pfb
    large_pfb.lib()
    return large_pfb


def test_header_declarations_equal_the_ctypes_signatures(large_pfb):
    header = open(os.path.join(ROOT, "include", STEM + ".h")).read()
    for phrase in ("Out of scope", "N <= 4096", "real-valued input", "oversampled", "complex prototypes", "synthesis"):
        assert phrase in header, phrase
    decl = ac.declarations(STEM + ".h")
    assert sorted(decl) == sorted(large_pfb.SIGS) == sorted(NAMES)
    for name, (res, args) in decl.items():
        assert large_pfb.SIGS[name] == ac.signature(res, args), name
    # launch_tuned = the arguments of launch + schedule + max_workgroups; benchmark = launch with the timer in the stream's place; and the
    # three shared entry points are the complex bank's, word for word, under the new names
    assert large_pfb.SIGS[STEM + "_launch_tuned"][1] == large_pfb.SIGS[STEM + "_launch"][1] + [ctypes.c_int, ctypes.c_int]
    assert large_pfb.SIGS[STEM + "_benchmark"][1][:-1] == large_pfb.SIGS[STEM + "_launch"][1][:-1]
    small = ac.declarations("smfft_pfb.h")
    for f in ("frames", "launch", "benchmark"):
        assert re.sub(r"\s+", " ", small["smfft_pfb_" + f][1]) == re.sub(r"\s+", " ", decl[f"{STEM}_{f}"][1]), f
    assert large_pfb.SIZES == SIZES == linv.SIZES


def test_library_exports_exactly_the_five_symbols(large_pfb):
    nm = subprocess.run(["nm", "-D", "--defined-only", large_pfb.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r" T (smfft_\w+)$", nm, re.M)) == sorted(NAMES)


def test_abi_frames(large_pfb):
    assert large_pfb.lib().smfft_large_pfb_frames(10 * 8192, 8192, 4) == 7


def test_unsupported_combinations_return_minus_one_without_a_device(large_pfb):
    """all validation happens before any HIP call: these return -1 (or 0 when there is no whole frame) with no device and null pointers"""
    lib = large_pfb.lib()
    frames, launch, benchmark, launch_tuned, default_schedule = (getattr(lib, name) for name in NAMES)
    t = ctypes.c_double(0.0)
    L = 1 << 22
    bad = [(L, 1, n, 4) for n in (0, 1024, 4096, 8191, 32768, -8192)] + [(L, 1, 8192, p) for p in (0, 33, -1)]
    bad += [(L, c, 16384, 4) for c in (0, -1)] + [(-1, 1, 8192, 4), (-5, 2, 16384, 1)]
    for L_, C, N, P in bad:
        for power in (0, 1):
            assert launch(None, L_, C, None, N, P, power, None, None) == -1, (L_, C, N, P)
            assert launch_tuned(None, L_, C, None, N, P, power, None, None, 1, 8) == -1, (L_, C, N, P)
            assert benchmark(None, L_, C, None, N, P, power, None, ctypes.byref(t)) == -1, (L_, C, N, P)
    for N in SIZES:
        for schedule, max_workgroups in ((-1, 0), (3, 0), (0, -1), (2, -8)):
            assert launch_tuned(None, L, 1, None, N, 4, 0, None, None, schedule, max_workgroups) == -1, (N, schedule, max_workgroups)
        # no whole frame is not an error: nothing is launched
        for L_ in (0, N - 1, 4 * N - 1):
            for power in (0, 1):
                assert launch(None, L_, 2, None, N, 4, power, None, None) == 0
                assert launch_tuned(None, L_, 2, None, N, 4, power, None, None, 2, 16) == 0
                assert benchmark(None, L_, 2, None, N, 4, power, None, ctypes.byref(t)) == 0
    assert t.value == 0.0
    for n in (0, 1024, 4096, 32768):
        assert frames(L, n, 4) == -1 and default_schedule(n, 4) == -1
    for p in (0, 33, -1):
        assert frames(L, 8192, p) == -1 and default_schedule(16384, p) == -1
    assert frames(-1, 8192, 4) == -1
    with pytest.raises(ValueError):
        large_pfb.frames(1000, 4096, 4)
    with pytest.raises(ValueError):
        large_pfb.default_schedule(8192, 33)
    with pytest.raises(RuntimeError):
        large_pfb.launch(None, L, 1, None, 4096, 4, None)
    with pytest.raises(RuntimeError):
        large_pfb.launch_tuned(None, L, 1, None, 8192, 4, None, schedule=3)
    with pytest.raises(ValueError):
        large_pfb.channelize(np.zeros(4096, np.complex64), np.zeros(4 * 4096, np.float32), 4096)
    with pytest.raises(ValueError):
        large_pfb.channelize(np.zeros(16384, np.complex64), np.zeros(8192, np.complex64), 8192)
    assert large_pfb.channelize(np.zeros((2, 9000), np.complex64), np.zeros(2 * 8192, np.float32), 8192).shape == (2, 0, 8192)
    # and the small banks keep their limit
    from smfft_amd import pfb
    assert pfb.lib().smfft_pfb_launch(None, L, 1, None, 8192, 4, 0, None, None) == -1


def test_frames_and_default_schedule(large_pfb):
    for N in SIZES:
        for P in (1, 4, 32):
            assert large_pfb.default_schedule(N, P) in (large_pfb.STRIDE, large_pfb.XCD_BLOCKED)
            for L in (0, N - 1, P * N - 1, P * N, P * N + 1, (P + 9) * N + N - 1, (1 << 34) + 5):
                assert large_pfb.frames(L, N, P) == max(L // N - P + 1, 0) == lpm.frames(L, N, P)


def test_prototype(large_pfb):
    from smfft_amd import pfb
    for N, P in ((8192, 1), (8192, 4), (16384, 8), (16384, 3)):
        h = large_pfb.prototype(N, P)
        M = P * N
        assert h.dtype == np.float32 and h.shape == (M,)
        assert np.array_equal(h, h[::-1]), "symmetric to the bit"
        assert h[M // 2 - 1] == h[M // 2] == h.max()
        want = lpm.hamming_prototype(N, P)
        assert np.array_equal(h, want.astype(np.float32)) or np.max(np.abs(h.astype(np.float64) - want)) <= 2.0 ** -24 * np.max(np.abs(want))
        assert np.array_equal(h, pfb.prototype(N, P)), "the complex bank's prototype"
    with pytest.raises(ValueError):
        large_pfb.prototype(8192, 2, "kaiser")


def test_import_does_not_load_the_library():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import smfft_amd, smfft_amd.large_pfb as l; "
            "maps = open('/proc/self/maps').read(); assert 'libsmfft_large_pfb' not in maps; print('ok')")
    p = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout + p.stderr


# ------------------------------------------------------------------------------------------------ kernel inventory
def test_every_kernel_is_in_the_inventory_with_its_tests(large_pfb):
    ac.check_inventory(large_pfb.LIB_PATH, linv.KERNELS, "smfft_large_pfb_", 4)


# ------------------------------------------------------------------------------------------------ leakage
from tests.pfb_gpu_harness import LEAKAGE  # noqa: E402  (the figures the GPU test holds the device to as well)


@pytest.mark.parametrize("N", SIZES)
def test_leakage_of_an_off_centre_tone(N):
    rect = float(lpm.leakage_of(np.abs(np.fft.fft(lpm.tone(N, N))) ** 2, 100))
    assert abs(rect - 0.60) < 0.01
    assert sorted(LEAKAGE) == list(range(1, 33))
    for P, want in LEAKAGE.items():
        got = lpm.leakage(N, P)
        print(f"N={N} P={P}: leakage {got:.3g} (plain FFT {rect:.3g})")
        assert abs(got - want) <= 0.01 * want, (N, P, got, want)
        assert (got < rect) == (P >= 2), (N, P)

"""The polyphase filter bank channelizer (smfft_amd/csrc/smfft_pfb.hip, smfft_pfb.hpp, include/smfft_pfb.h) on the CPU: the fp64 model's
two forms of the definition agree, the header's PfbPlan compiled for the host gives the model's frames, tiles, offsets and schedule,
the replay of the kernel's loop stores every output once and loads inside its own stream's window, the gfx950 code keeps the
library's rules (no scratch, no v_sin / v_cos, no packed f32, the sixteen signal loads of a tap together), the C ABI declares, exports
and validates without a device, every shipped kernel is in tests/pfb_inventory.py with its tests, and the leakage property the GPU test relies on holds for the model.  No GPU code is run (hipcc
cross-compiles gfx950)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pfb_model as pm  # noqa: E402

from tests import addon_checks as ac  # noqa: E402
from tests import pfb_inventory as pinv  # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "smfft_amd", "csrc")
SIZES = (256, 512, 1024, 2048, 4096)
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def _rand(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# ------------------------------------------------------------------------------------------------ the model
def test_models_two_forms_agree():
    rng = np.random.default_rng(0)
    N = 256
    for P, C, L in ((1, 1, 256), (2, 2, 5 * 256 + 17), (4, 1, 7 * 256 + 255), (32, 1, 34 * 256 + 3)):
        x, h = _rand(rng, (C, L)), rng.standard_normal(P * N)
        a, b = pm.pfb(x, h, N), pm.pfb_direct(x, h, N)
        assert a.shape == (C, L // N - P + 1, N)
        assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b)), (P, C, L)


@pytest.mark.parametrize("N", [256, 1024, 4096])
def test_model_with_one_tap_of_ones_is_the_plain_fft(N):
    rng = np.random.default_rng(N)
    x = _rand(rng, (2, 5 * N + 11))
    want = np.fft.fft(x[:, :5 * N].reshape(2, 5, N), axis=-1)
    got = pm.pfb(x, np.ones(N), N)
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
    assert np.allclose(pm.pfb(x, np.ones(N), N, power=True), np.abs(want) ** 2, rtol=1e-12)


# ------------------------------------------------------------------------------------------------ header == model
def _plan_cases():
    cases = []
    for N in SIZES:
        per = 4096 // N
        for P in (1, 4, 32):
            for L in (0, P * N - 1, P * N, P * N + 1, (P + 2) * N + N // 2, (P + per) * N + 7, (P + 2 * per + 1) * N - 1):
                for C in (1, 3):
                    cases.append((L, N, P, C))
    # F not a multiple of 4096 / N with three streams: tiles straddle streams
    cases += [(P * 256 + 17 * 256 + 5, 256, P, 3) for P in (2, 8)] + [((4 + 2) * 1024 + 1, 1024, 4, 3)]
    # C F N and C L beyond 2^32
    cases += [((1 << 31) + 12345, 1024, 4, 2), ((1 << 33) + 7, 4096, 16, 3), ((1 << 32) + 255, 256, 32, 5)]
    return cases


@needs_hipcc
def test_header_plan_is_the_models(tmp_path):
    src = tmp_path / "pfb_plan.hip"
    src.write_text(r'''
#include <cstdio>
#include "smfft_pfb.hpp"
int main(int argc, char**) {
    long long L; int N, P, C;
    if (argc == 1) {
        while (scanf("%lld %d %d %d", &L, &N, &P, &C) == 4) {
            const smfft::PfbPlan w{L, N, P, C};
            const long long pairs = w.pairs(), tiles = w.tiles();
            printf("F %lld %lld %d %lld\n", w.frames(), pairs, w.per_tile(), tiles);
            const long long probe[8] = {0, 1, w.frames() - 1, w.frames(), pairs / 2, pairs - 2, pairs - 1, (1ll << 31) / N + 1};
            for (long long g : probe) {
                if (g < 0 || g >= pairs) continue;
                printf("%lld %lld %lld %lld %lld\n", g, w.stream_of(g), w.frame_of(g), w.input_offset(g), w.output_offset(g));
            }
            if (tiles > 0) {
                printf("T");
                for (int j = 0; j < w.per_tile(); ++j) printf(" %lld", w.pair_of(tiles - 1, j));
                printf("\n");
            }
        }
        return 0;
    }
    long long G, R;
    while (scanf("%lld %d %d %d %lld %lld", &L, &N, &P, &C, &G, &R) == 6) {
        const smfft::PfbPlan w{L, N, P, C};
        const long long grid = w.grid(G, R), runs = w.runs(R);
        printf("S %lld %lld %lld\n", w.run_length(R), runs, grid);
        for (long long b = 0; b < grid; ++b) {
            if (grid > 6 && b > 2 && b < grid - 2) continue;
            printf("%lld:", b);
            int shown = 0;
            for (long long j = b; j < runs && shown < 4; j += grid, ++shown) printf(" %lld-%lld", w.run_begin(j, R), w.run_end(j, R));
            printf("\n");
        }
    }
    return 0;
}
''')
    exe = tmp_path / "pfb_plan"
    subprocess.check_call([HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I" + CSRC, str(src), "-o", str(exe)], stderr=subprocess.DEVNULL)
    cases = _plan_cases()
    out = subprocess.run([str(exe)], input="".join("%d %d %d %d\n" % c for c in cases), capture_output=True, text=True, check=True).stdout.split("\n")
    want = []
    for L, N, P, C in cases:
        w = pm.Plan(L, N, P, C)
        F, pairs, tiles = w.frames(), w.pairs(), w.tiles()
        assert F == max(L // N - P + 1, 0) and tiles == -(-(C * F) // (4096 // N))
        want.append(f"F {F} {pairs} {w.per_tile()} {tiles}")
        for g in (0, 1, F - 1, F, pairs // 2, pairs - 2, pairs - 1, (1 << 31) // N + 1):
            if 0 <= g < pairs:
                want.append(f"{g} {w.stream_of(g)} {w.frame_of(g)} {w.input_offset(g)} {w.output_offset(g)}")
        if tiles:
            want.append("T " + " ".join(str(w.pair_of(tiles - 1, j)) for j in range(w.per_tile())))
    assert [line for line in out if line] == want
    # the cases the issue names are in the grid
    assert any(pm.Plan(*c).frames() == 0 and c[0] > 0 for c in cases) and any(pm.Plan(*c).frames() == 1 for c in cases)
    assert any(c[3] == 3 and pm.Plan(*c).frames() % pm.Plan(*c).per_tile() for c in cases)
    assert any(pm.Plan(*c).pairs() * c[1] > 1 << 32 and c[0] * c[3] > 1 << 32 for c in cases)

    sched = []
    for L, N, P, C in ((40 * 1024 + 3, 1024, 4, 3), (300 * 256, 256, 8, 1), (9 * 4096, 4096, 2, 2), ((1 << 31) + 12345, 1024, 4, 2)):
        tiles = pm.Plan(L, N, P, C).tiles()
        for R in (1, 3, 16, tiles + 5):
            for G in (1, 5, max(1, tiles // 3), tiles, tiles + 9, 768):
                sched.append((L, N, P, C, G, R))
    out = subprocess.run([str(exe), "schedule"], input="".join("%d %d %d %d %d %d\n" % c for c in sched), capture_output=True, text=True,
                         check=True).stdout.split("\n")
    want = []
    for L, N, P, C, G, R in sched:
        w = pm.Plan(L, N, P, C)
        grid, runs = w.grid(G, R), w.runs(R)
        want.append(f"S {w.run_length(R)} {runs} {grid}")
        for b in range(grid) if grid <= 6 else (0, 1, 2, grid - 2, grid - 1):
            js = list(range(b, runs, grid))[:4]
            want.append(f"{b}:" + "".join(f" {w.run_begin(j, R)}-{w.run_end(j, R)}" for j in js))
    assert [line for line in out if line] == want


def test_schedule_visits_every_tile_once():
    for L, N, P, C in ((40 * 1024 + 3, 1024, 4, 3), (300 * 256, 256, 8, 1), (9 * 4096, 4096, 2, 2)):
        w = pm.Plan(L, N, P, C)
        tiles = w.tiles()
        for R in (1, 3, 16, tiles + 5):
            for G in (1, 5, tiles, tiles + 9):
                grid = w.grid(G, R)
                assert 1 <= grid <= min(G, tiles)
                sched = w.schedule(grid, R)
                assert all(sched), "a workgroup of the grid without work"
                assert sorted(t for mine in sched for t in mine) == list(range(tiles)), (L, N, P, C, R, G)


# ------------------------------------------------------------------------------------------------ the replay
@pytest.mark.parametrize("case", [(7 * 256 + 100, 256, 4, 3), (5 * 512, 512, 1, 1), (12 * 1024 + 1023, 1024, 8, 3), (40 * 2048, 2048, 32, 2),
                                  (6 * 4096 + 5, 4096, 2, 3), (3 * 4096, 4096, 4, 2)])
def test_replay_stores_once_and_loads_inside_the_window(case):
    L, N, P, C = case
    w = pm.Plan(L, N, P, C)
    F = w.frames()
    if F == 0:
        assert w.tiles() == 0
        return
    for G, R in ((3, 1), (2, 3), (w.tiles() + 4, 16)):
        loads, stores, taps = pm.replay(w, w.grid(G, R), R)
        assert np.array_equal(np.sort(stores), np.arange(C * F * N)), "every output element exactly once"
        assert taps == P * N - 1
        for pair, c, addr in loads:
            assert addr.shape == (P, N)
            assert addr.min() >= c * L and addr.max() < c * L + (F + P - 1) * N, (case, pair)
            if pair >= 0:
                f = pair - c * F
                assert np.array_equal(np.sort(addr, axis=1), c * L + (f + np.arange(P))[:, None] * N + np.arange(N)[None, :])


# ------------------------------------------------------------------------------------------------ gfx950 code
@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return ac.addon_isa("smfft_pfb", "PFB", ac.PFB_SIZES, tmp_path_factory.mktemp("pfb_isa"))


def test_pfb_kernels_have_no_scratch_no_transcendentals_no_packed_f32(isa):
    ac.check_pfb_kernel_rules(isa, "pfb_kernel")


def test_pfb_signal_loads_of_a_tap_are_issued_together(isa):
    """the signal loads are the kernel's only 8-byte global loads through a vector address: the twiddle tables are read through scalar
    bases, the coefficients are 4-byte loads"""
    ac.check_pfb_signal_loads(isa, "pfb_kernel", signal=r"global_load_dwordx2 v\[\d+:\d+\], v\[\d+:\d+\], off", tap=r"global_load_dword ",
                              arithmetic=r"(v_add|v_addc|v_lshl|v_lshlrev|v_mov|v_mad|v_ashr|v_and|v_or|s_add|s_addc|s_lshl|s_mov|s_nop|s_mul|;)")


# ------------------------------------------------------------------------------------------------ C ABI
@pytest.fixture(scope="module")
def pfb():
    from smfft_amd import pfb
    pfb.lib()
    return pfb


def test_header_declarations_equal_the_ctypes_signatures(pfb):
    ac.check_pfb_declarations(pfb, "smfft_pfb", ("Out of scope", "oversampled", "real-valued input", "complex prototypes", "synthesis", "N <= 128", "N >= 8192"))
    assert pfb.SIZES == SIZES


def test_library_exports_exactly_the_five_symbols(pfb):
    ac.check_pfb_exports(pfb, "smfft_pfb")
    # and libsmfft_amd.so keeps its list: nothing of the filter bank went into it
    import smfft_amd
    nm = subprocess.run(["nm", "-D", "--defined-only", smfft_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.findall(r"pfb", nm)


def test_unsupported_combinations_return_minus_one_without_a_device(pfb):
    ac.check_pfb_rejections(pfb, "smfft_pfb", samples=1, bad_lengths=[(-1, 1, 1024, 4)])
    with pytest.raises(ValueError):
        pfb.frames(1000, 100, 4)
    with pytest.raises(RuntimeError):
        pfb.launch(None, 1 << 20, 1, None, 8192, 4, None)
    with pytest.raises(ValueError):
        pfb.channelize(np.zeros(4096, np.complex64), np.zeros(100, np.float32), 256)
    with pytest.raises(ValueError):
        pfb.channelize(np.zeros(4096, np.complex64), np.zeros(256, np.complex64), 256)
    assert pfb.channelize(np.zeros((2, 1000), np.complex64), np.zeros(1024, np.float32), 256).shape == (2, 0, 256)


def test_frames_and_default_tile_run(pfb):
    for N in SIZES:
        for P in (1, 4, 32):
            assert pfb.default_tile_run(N, P) >= 1
            for L in (0, N - 1, P * N - 1, P * N, P * N + 1, (P + 9) * N + N - 1, (1 << 33) + 5):
                assert pfb.frames(L, N, P) == max(L // N - P + 1, 0) == pm.frames(L, N, P)


def test_prototype(pfb):
    for N, P in ((256, 1), (256, 4), (1024, 8), (4096, 32), (512, 3)):
        h = pfb.prototype(N, P)
        M = P * N
        assert h.dtype == np.float32 and h.shape == (M,)
        assert np.array_equal(h, h[::-1]), "symmetric to the bit"
        assert h[M // 2 - 1] == h[M // 2] == h.max()
        m = np.arange(M, dtype=np.float64)
        want = np.sinc((m - (M - 1) / 2) / N) * (0.54 - 0.46 * np.cos(2 * np.pi * m / (M - 1)))
        assert np.array_equal(h, want.astype(np.float32)) or np.max(np.abs(h.astype(np.float64) - want)) <= 2.0 ** -24 * np.max(np.abs(want))
    assert np.array_equal(pfb.prototype(256, 2, "rectangular"), np.sinc((np.arange(512) - 255.5) / 256).astype(np.float32))
    with pytest.raises(ValueError):
        pfb.prototype(256, 2, "kaiser")


# ------------------------------------------------------------------------------------------------ kernel inventory
def test_every_pfb_kernel_is_in_the_inventory_with_its_tests(pfb):
    """the rule of tests/test_kernel_inventory.py, without the "host" kind (tests/pfb_inventory.py says why)"""
    ac.check_inventory(pfb.LIB_PATH, pinv.KERNELS, "smfft_pfb_", 10, kinds=("tests", "bounds", "probes"))


# ------------------------------------------------------------------------------------------------ leakage
def leakage(power, channel):
    """(power outside `channel`) / (power in it), per spectrum"""
    power = np.asarray(power, np.float64)
    return (power.sum(axis=-1) - power[..., channel]) / power[..., channel]


def tone(N, length, channel=100.37, amplitude=1.0):
    return amplitude * np.exp(2j * np.pi * channel * np.arange(length) / N)


@pytest.mark.parametrize("N", [256, 1024, 4096])
def test_filter_bank_leaks_less_than_the_plain_fft(N):
    """a unit tone at channel 100.37 through a Hamming prototype: the PFB frame's power outside channel 100 over the power inside is
    below the plain FFT's of one frame (0.60), the more so the longer the prototype: 0.33, 0.098, 5.6e-3, 5.4e-6, 8.9e-7 for
    P = 2 ... 32, the same at all three N"""
    expected = {2: 0.33, 4: 0.098, 8: 5.6e-3, 16: 5.4e-6, 32: 8.9e-7}
    rect = leakage(np.abs(np.fft.fft(tone(N, N))) ** 2, 100)
    assert abs(rect - 0.60) < 0.01
    m = np.arange(N, dtype=np.float64)
    for P, want in expected.items():
        M = P * N
        mm = np.arange(M, dtype=np.float64)
        h = np.sinc((mm - (M - 1) / 2) / N) * np.hamming(M)
        got = leakage(pm.pfb(tone(N, M), h, N, power=True)[0, 0], 100)
        print(f"N={N} P={P}: leakage {got:.3g} (plain FFT {rect:.3g})")
        assert got < rect
        assert abs(got - want) <= 0.05 * want, (N, P, got, want)
    del m

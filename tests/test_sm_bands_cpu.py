"""CPU checks of the band-spectrogram library (smfft_amd/csrc/smfft_bands.hip, libsmfft_bands.so): the model (tools/bands_model.py on
tools/stft_model.py) in fp64 is the dense product of the definition, the mel filter bank of smfft_amd.bands is the triangular filters
written out by definition here, and the staged fp32 model -- every product and partial sum rounded, sequential in bin order -- stays
inside the GPU tests' bounds; the gfx950 code of the five kernels keeps its budget; and the C ABI declares, exports and validates the
eight entry points without a device, the plan's layout included.  No GPU code is run (hipcc cross-compiles gfx950)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bands_model as bm  # noqa: E402
import stft_model as sm  # noqa: E402

from tests import addon_checks as ac  # noqa: E402
from tests import bands_inventory  # noqa: E402
from tests.fir_gpu_harness import ROW_MAX, ROW_REL_L2  # noqa: E402

CSRC = ac.CSRC
LIB = os.path.join(ROOT, "smfft_amd", "libsmfft_bands.so")
SIZES = (256, 512, 1024, 2048, 4096)
LENGTHS = (512, 1024, 2048, 4096, 8192)
NAMES = tuple("smfft_bands_" + f for f in ("fft_size", "frames", "plan_bytes", "tables", "prepare", "launch", "launch_tuned", "benchmark"))
LDS_BUDGET = 34816 + 45056     # 4096 / 16 * 17 float2, the transform region of 4096 points, and 11,264 words of staged plan behind it
NO_DEVICE = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


@pytest.fixture(scope="module")
def bands_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", CSRC, "-j", "4", "../libsmfft_bands.so"])
    return LIB


@pytest.fixture(scope="module")
def bd(bands_lib):
    from smfft_amd import bands
    bands.lib()
    return bands


def _random_table(rng, n, bands, longest):
    bins = n // 2 + 1
    count = rng.integers(0, longest + 1, bands)
    count[0] = 0                                            # an empty band
    first = np.array([rng.integers(0, bins - c + 1) for c in count])
    return first, count, rng.standard_normal(int(count.sum())).astype(np.float32)


# ---- 1: the model -------------------------------------------------------------------------------------------
def test_fp64_model_is_the_dense_product():
    """n = 512, 2 x 3 frames, with a window that has no symmetry and without one: the band sums of the fp64 chain within 1e-12 of the
    dense product W |X|^2 with X from the O(n^2) sums of the definition; overlapping, empty and negative bands"""
    n = 512
    rng = np.random.default_rng(280)
    fr = rng.standard_normal((2, 3, n)).astype(np.float32)
    table = _random_table(rng, n, 19, 40)
    W = bm.dense(n, *table)
    assert W.shape == (19, n // 2 + 1) and (W < 0).any() and (W > 0).any()
    ramp = sm.hann(n) * (1 + np.arange(n) / (2 * n)) + 0.1
    for win in (None, ramp):
        got = bm.bands(fr, *table, win)
        P = np.abs(sm.direct(fr, win)) ** 2
        want, A = P @ W.T, P @ np.abs(W).T
        assert got.shape == (2, 3, 19) and got.dtype == np.float64
        l2, mx = bm.errors(got, want, A)
        print(f"fp64 model against the dense product: relL2 = {l2.max():.2e}, max = {mx.max():.2e}")
        assert l2.max() <= 1e-12 and mx.max() <= 1e-12
    # the sequential stage: -0 + t_0 + t_1 ..., an empty band +0, the identity table the powers themselves
    p = rng.standard_normal((4, n // 2 + 1)).astype(np.float32) ** 2
    ident = (np.arange(n // 2 + 1), np.ones(n // 2 + 1, int), np.ones(n // 2 + 1, np.float32))
    assert np.array_equal(bm.sequential(p, *ident).view(np.uint32), p.view(np.uint32))
    three = bm.sequential(p, [2, 9], [3, 0], np.array([0.5, -2.0, 3.0], np.float32))
    want = ((np.float32(0.5) * p[:, 2] + np.float32(-2.0) * p[:, 3]).astype(np.float32) + np.float32(3.0) * p[:, 4]).astype(np.float32)
    assert np.array_equal(three[:, 0].view(np.uint32), want.view(np.uint32)) and not three[:, 1].view(np.uint32).any()


def _mel_by_definition(n, rate, n_mels, f_min, f_max, scale, norm):
    """torchaudio.functional.melscale_fbanks, transposed, one entry at a time"""
    import math

    def to_mel(f):
        if scale == "htk":
            return 2595.0 * math.log10(1.0 + f / 700.0)
        return f / (200.0 / 3.0) if f < 1000.0 else 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0)

    def to_hz(m):
        if scale == "htk":
            return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
        return (200.0 / 3.0) * m if m < 15.0 else 1000.0 * math.exp((math.log(6.4) / 27.0) * (m - 15.0))
    lo, hi = to_mel(f_min), to_mel(f_max)
    pts = [to_hz(lo + (hi - lo) * j / (n_mels + 1)) for j in range(n_mels + 2)]
    W = np.zeros((n_mels, n // 2 + 1))
    for b in range(n_mels):
        for k in range(n // 2 + 1):
            f = k * (rate / 2.0) / (n // 2)
            v = max(0.0, min((f - pts[b]) / (pts[b + 1] - pts[b]), (pts[b + 2] - f) / (pts[b + 2] - pts[b + 1])))
            W[b, k] = v * (2.0 / (pts[b + 2] - pts[b]) if norm == "slaney" else 1.0)
    return W


@pytest.mark.parametrize("norm", [None, "slaney"])
@pytest.mark.parametrize("scale", ["htk", "slaney"])
def test_mel_filterbank_is_the_definition(scale, norm):
    """mel_filterbank against the triangular filters written out entry by entry, on both mel scales, with and without the Slaney
    norm, with the default range and with f_min / f_max inside it; and against from_dense expanded back to a dense matrix"""
    from smfft_amd import bands
    for n, rate, n_mels, f_min, f_max in ((512, 16000, 40, 0.0, None), (1024, 22050, 23, 60.0, 7600.0)):
        got = bands.mel_filterbank(n, rate, n_mels, f_min, f_max, scale, norm)
        want = _mel_by_definition(n, rate, n_mels, f_min, rate / 2.0 if f_max is None else f_max, scale, norm)
        assert got.shape == (n_mels, n // 2 + 1) and got.dtype == np.float64
        assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, want.max()), (n, scale, norm, np.max(np.abs(got - want)))
        assert got.min() >= 0.0 and (got.max(axis=1) > 0).all()
        first, count, w = bands.from_dense(n, got)
        assert w.dtype == np.float32 and first.dtype == count.dtype == np.int32 and count.sum() == w.size <= 4 * (n // 2 + 1)
        assert np.array_equal(bands.to_dense(n, first, count, w, np.float32), got.astype(np.float32))
        assert np.array_equal(bm.dense(n, first, count, w), got.astype(np.float32).astype(np.float64))
        # the support runs from the first to the last non-zero entry
        for b in range(n_mels):
            nz = np.flatnonzero(got[b])
            assert first[b] == nz[0] and count[b] == nz[-1] - nz[0] + 1
    with pytest.raises(ValueError):
        bands.mel_filterbank(512, 16000, 40, mel_scale="bark")
    with pytest.raises(ValueError):
        bands.mel_filterbank(512, 16000, 40, norm="area")
    with pytest.raises(ValueError):
        bands.mel_filterbank(512, 16000, 40, 9000.0)
    with pytest.raises(ValueError):
        bands.mel_filterbank(500, 16000, 40)


def test_from_dense_and_uniform_bands():
    """from_dense keeps the zeros inside a support, makes a row of zeros an empty band and refuses a dense matrix; uniform_bands
    re-bins with a shorter last band"""
    from smfft_amd import bands
    n, bins = 512, 257
    W = np.zeros((4, bins))
    W[0, 3], W[0, 7] = 1.5, -2.0
    W[2, 256] = 4.0
    W[3, :] = 1.0
    first, count, w = bands.from_dense(n, W)
    assert first.tolist() == [3, 0, 256, 0] and count.tolist() == [5, 0, 1, 257] and w[:6].tolist() == [1.5, 0, 0, 0, -2.0, 4.0]
    assert bands.from_dense(n, np.ones((4, bins)))[1].sum() == 4 * bins                    # exactly at the cap
    for bad in (np.ones((5, bins)), np.ones((4, bins - 1)), np.ones(bins), np.ones((bins + 1, bins)), np.zeros((0, bins))):
        with pytest.raises(ValueError):
            bands.from_dense(n, bad)
    first, count, w = bands.uniform_bands(n, 10)
    assert first.tolist() == list(range(0, 257, 10)) and count.tolist() == [10] * 25 + [7] and w.tolist() == [1.0] * 257
    assert bands.uniform_bands(n, 257)[1].tolist() == [257] and bands.uniform_bands(n, 1)[1].tolist() == [1] * 257
    for width in (0, 258):
        with pytest.raises(ValueError):
            bands.uniform_bands(n, width)


def test_staged_fp32_model_is_inside_the_bounds():
    """every stage of the chain rounded to fp32, every product w * p rounded and the sums sequential in fp32, Hann-windowed Gaussian
    noise under HTK mel tables of 40 bands at 16 kHz at every n and of 128 bands at n = 8192: inside kappa_2 2 ROW_REL_L2 + (Lmax + 1)
    2^-24 and kappa_inf 2 ROW_MAX + (Lmax + 1) 2^-24, the bounds of the GPU tests"""
    from smfft_amd import bands
    for n, n_mels in [(n, 40) for n in LENGTHS] + [(8192, 128)]:
        fr = np.random.default_rng(281 + n + n_mels).standard_normal((3, n)).astype(np.float32)
        w = sm.hann(n, np.float32)
        table = bands.from_dense(n, bands.mel_filterbank(n, 16000, n_mels))
        W = bm.dense(n, *table)
        P = sm.chain(fr, w, np.float64, power=True)
        k2, kinf, b2, binf = bm.bounds(W, P, int(table[1].max()), ROW_REL_L2, ROW_MAX)
        got = bm.bands(fr, *table, w, np.float32)
        assert got.dtype == np.float32 and np.array_equal(bm.bands(fr, *table, w), P @ W.T)
        l2, mx = bm.errors(got, P @ W.T, P @ np.abs(W).T)
        print(f"n={n} mel {n_mels}: Lmax = {table[1].max()}, kappa_2 = {k2.max():.2f}, kappa_inf = {kinf.max():.2f}; staged fp32 model relL2 = {l2.max():.2e} "
              f"(bound {b2.min():.1e}), max = {mx.max():.2e} (bound {binf.min():.1e})")
        assert np.all(l2 <= b2) and np.all(mx <= binf), (n, n_mels)
        assert np.all(k2 >= 1.0 - 1e-12)                      # ||A||_2 = ||W P||_2 <= ||W||_2 ||P||_2 for W >= 0
    assert ROW_REL_L2 == 1e-6 and ROW_MAX == 5e-6


def test_source_repeats_the_stft_step_and_builds_on_the_shared_layers():
    """the frame-to-spectrum statements of smfft_stft.hip stand in smfft_bands.hip as they are (DESIGN.md sections 27 and 28 say why
    they are written three times); the twiddle row comes from the shared table; the sample loads go through rows::gload2; the entry
    points are the shared host layer's; nothing transcendental, no atomics, no allocation"""
    source, stft = open(os.path.join(CSRC, "smfft_bands.hip")).read(), open(os.path.join(CSRC, "smfft_stft.hip")).read()
    for line in ("for (int q = 0; q < 16; ++q) r[q] = gload2(xr + 2 * (fwd.u + T * q));", "for (int q = 0; q < 16; ++q) w[q] = wload2(window + 2 * (fwd.u + T * q));",
                 "fwd.transform(r, sf);", "for (int q = 0; q < 16; ++q) sf[fwd.u + T * q] = r[q];", "const float2* partner = sf + (T - fwd.u);",
                 "for (int q = 0; q < 16; ++q) p[q] = partner[T * (15 - q)];", "p[0] = self ? r[0] : p[0];", "const int u = per_tile(fwd.u);",
                 "const float2 w = row_entry(&rows<M>.wn[u + T * q]);",
                 "const float sx = r[q].x + p[q].x, sy = r[q].y - p[q].y, dx = r[q].x - p[q].x, dy = r[q].y + p[q].y;",
                 "r[q] = make_float2(0.5f * (sx - w.y * dx + w.x * dy), 0.5f * (sy - w.y * dy - w.x * dx));",
                 "const float x0 = p[0].x + p[0].y, xm = p[0].x - p[0].y;",
                 "r[0] = self ? make_float2(x0, 0.f) : r[0];", "const float pw = r[q].x * r[q].x + r[q].y * r[q].y;", "const float pm = xm * xm;",
                 "const float v0 = r[q].x * w[q].x;", "const float v1 = r[q].y * w[q].y;", "wn[k] = w32768(k * (16384 / M))",
                 "const long long c = gg / frames;", "const float* xr = in + c * stream_stride + (gg - c * frames) * hop;"):
        assert line in source and line in stft, line
    assert '#include "smfft_rows.hpp"' in source and '#include "smfft_rows_host.hpp"' in source and not re.search(r'#include "[^"]*\.inc"', source)
    assert "rows::gload2<SMFFT_BANDS_NT_LOAD != 0>" in source
    for f in ("checked_launch(", "checked_launch_tuned(", "checked_benchmark("):
        assert source.count(f) == 1, f
    code = re.sub(r"//[^\n]*", "", source)
    assert not re.search(r"\b(sinf?|cosf?|sincosf?|__sinf|__cosf|expf?|logf?|log10f?|powf?|sqrtf?)\s*\(", code)
    assert "atomic" not in code.lower() and "hipMalloc" not in source
    # each product a statement of its own, the sum from -0
    assert "const float t = wp[i] * pp[i];" in source and "acc = acc + t;" in source and "float acc = -0.f;" in source
    assert "## 28. Band spectrograms" in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---- 2: ISA budget and inventory -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """{M: assembly of smfft_bands_<M>.o as the Makefile compiles it}"""
    assert os.path.exists(ac.HIPCC), "hipcc is missing: the library cannot be built either"
    return ac.addon_isa("smfft_bands", "BANDS", SIZES, tmp_path_factory.mktemp("bands_isa"))


def test_isa_budget_of_what_ships(isa):
    """per M exactly one kernel, read from the compiled object's metadata: no scratch, at most 256 VGPRs (two waves per SIMD), static
    LDS of exactly 79,872 B -- the transform region and the staged plan behind it, the shipped choice; two workgroups per compute
    unit -- no transcendental and no atomic instruction, no flat access; two store instructions, the band loop's with the plan in LDS
    and with the plan in global memory, 4 bytes and non-temporal; plain loads: the samples, the window, the twiddle row and the plan"""
    total = 0
    for m, text in isa.items():
        descs = ac.descriptors(text)
        kernels = ac.pfb_kernels(text, r"\d+bands_kernel")
        assert len(descs) == 1 and set(descs) == set(kernels), (m, sorted(descs), sorted(kernels))
        total += len(descs)
        assert not re.search(r"\bscratch_", text), m
        for name, body in kernels.items():
            assert re.search(r"bands_kernelILi%dE" % m, name)
            # (v_rcp stays: the 64-bit division of the frame index by `frames`, stft_kernel's own statement)
            assert not [line for line in body if re.match(r"v_(sin|cos|exp|log|sqrt|rsq)_", line)], name
            assert not [line for line in body if re.match(r"(global|ds|flat|buffer)_atomic|flat_(load|store)", line)], name
            assert ac.descriptor_field(descs, name, "private_segment_fixed_size") == 0, name
            v, lds = ac.descriptor_field(descs, name, "next_free_vgpr"), ac.descriptor_field(descs, name, "group_segment_fixed_size")
            print(f"M={m}: bands_kernel: {v} VGPRs ({ac.occupancy(v)} waves per SIMD), {lds} B of LDS, 0 B of scratch")
            assert lds == LDS_BUDGET and 2 * lds <= ac.LDS_PER_CU, (name, lds)
            assert v <= 256 and ac.occupancy(v) >= 2, (name, v)
            loads = [i for i, line in enumerate(body) if line.startswith("global_load")]
            stores = [i for i, line in enumerate(body) if line.startswith("global_store")]
            assert not [i for i in loads if re.search(r"\bnt\b", body[i])], name           # the shipped policy: plain loads
            assert len(loads) >= 48 + 4, (name, len(loads))                                  # samples, window, W_n; first, count, offset, weights
            assert len(stores) == 2, (name, len(stores))
            assert all(re.match(r"global_store_dword\s", body[i]) and re.search(r"\bnt\b", body[i]) for i in stores), name
            assert min(stores) > min(loads), name
    assert total == 5


def test_library_ships_five_kernels_and_the_inventory_names_them(bands_lib):
    ac.check_inventory(bands_lib, bands_inventory.KERNELS, "smfft_", 5, kinds=("tests", "bounds", "probes"))
    assert len(bands_inventory.KERNELS) == 5
    assert all(e["call"].startswith("smfft_bands_launch") for e in bands_inventory.KERNELS.values())
    assert "permlane" in bands_inventory.__doc__ and "hostsim" in bands_inventory.__doc__ and "welch_inventory" in bands_inventory.__doc__


def test_isa_identity_compares_the_library():
    """tools/isa_identity.py compiles the five objects with the Makefile's flags and -I., like the other add-ons' (the tool itself
    needs the history of a git checkout and minutes of compiling: it is run by hand, DESIGN.md section 28 has its verdict)"""
    ac.check_isa_identity_lists("smfft_bands", "BANDS", SIZES)
    assert all("-ffp-contract=on" in ac.makefile_flags("BANDS", m) for m in SIZES)


# ---- 3: declarations and exports ---------------------------------------------------------------------------------
def test_python_mirror_matches_header(bands_lib):
    from smfft_amd import bands
    header = re.sub(r"[\s*]+", " ", open(os.path.join(ROOT, "include", "smfft_bands.h")).read())
    for phrase in ("P[k] = re re + im im, k = 0 ... M, is the value that smfft_stft_launch(kind = 1) stores for that frame, to the bit",
                   "1 <= bands <= M + 1", "0 <= first[b], 0 <= count[b] and first[b] + count[b] <= M + 1", "weights = sum of count[b] <= 4 (M + 1)",
                   "Bands may overlap, be empty or have negative weights", "out[(c frames + f) bands + b] = sum_i weight[b][i] P[first[b] + i]",
                   "written exactly once", "An empty band stores exactly +0", "Each product is a statement of its own",
                   "Summation order: one thread per band, sequentially in ascending bin order, starting from -0", "It is fixed by the plan and n alone",
                   "With the identity table (bands = M + 1, first[b] = b, count[b] = 1, weight 1.0) the output equals smfft_stft_launch(kind = 1) bit for bit",
                   "NULL means all ones", "plan_bytes = 12 bands + 4 weights bytes", "int32 first[bands], count[bands], offset[bands]",
                   "The plan is written by smfft_bands_tables / smfft_bands_prepare only", "the kernel trusts it",
                   "No workspace, no atomics, no transcendental and no allocation in a launch",
                   "The output may overlap neither the extent of the signal, nor the window, nor the plan's plan_bytes",
                   "allocate nothing and do not synchronise", "it is not graph-capturable", "Not graph-capturable", "Host only, no HIP call",
                   "not on the batch, the frame's position in it, the hop, the stream or the grid", "A NaN or Inf stays in the frames that contain the sample",
                   "bands outside 1 ... M + 1", "weights outside 0 ... 4 (M + 1)", "hop < 1", "stream_stride < 1",
                   "beyond 2^59 elements (computed in 128 bits)", "grid < 1 (launch_tuned)", "a forbidden overlap",
                   "A zero count launches nothing and returns 0", "Out of scope", "log, dB or a DCT (MFCC) in the kernel", "sums over frames combined with bands",
                   "complex or magnitude (|X|, not |X|^2) band inputs", "dense matrices", "n < 512", "not a power of two"):
        assert re.sub(r"[\s*]+", " ", phrase) in header, phrase
    decl = ac.declarations("smfft_bands.h")
    assert sorted(decl) == sorted(bands.SIGS) == sorted(NAMES)
    for name, (res, args) in decl.items():
        assert bands.SIGS[name] == ac.signature(res, args), name
    assert bands.SIZES == SIZES and bands.LENGTHS == LENGTHS
    for f in ("prepare", "prepare_ptr", "tables", "plan_bytes", "from_dense", "to_dense", "mel_filterbank", "uniform_bands", "launch_ptr", "benchmark", "launch",
              "band_spectrogram", "mel_spectrogram", "mel_plan", "frames", "fft_size", "hann", "Plan"):
        assert callable(getattr(bands, f)), f


def test_library_exports_exactly_the_eight_symbols(bands_lib):
    ac.check_exports(bands_lib, NAMES)
    assert len(NAMES) == 8


# ---- 4: the plan, on the host ----------------------------------------------------------------------------------------
def test_tables_and_plan_bytes_check_every_rule(bd):
    """smfft_bands_plan_bytes and smfft_bands_tables, host only: every rule of the header at its boundary and one past it, and the
    plan's layout read back -- int32 first[], count[], offset[] (prefix sums), then the weights as they were given"""
    L = bd.lib()
    for n in LENGTHS:
        M = n // 2
        assert L.smfft_bands_plan_bytes(n, 1, 0) == 12 and L.smfft_bands_plan_bytes(n, M + 1, 4 * (M + 1)) == 12 * (M + 1) + 16 * (M + 1)
        assert L.smfft_bands_plan_bytes(n, 40, 1000) == 12 * 40 + 4 * 1000
        for bands, weights in ((0, 0), (-1, 0), (M + 2, 0), (1, -1), (1, 4 * (M + 1) + 1), (2 ** 31 - 1, 2 ** 31 - 1)):
            assert L.smfft_bands_plan_bytes(n, bands, weights) == -1, (n, bands, weights)
    for n in (256, 500, 16384, 0, -512, 513):
        assert L.smfft_bands_plan_bytes(n, 1, 1) == -1 and L.smfft_bands_fft_size(n) == -1 and L.smfft_bands_frames(1 << 20, n, 128) == -1
    assert [L.smfft_bands_fft_size(n) for n in LENGTHS] == list(SIZES)
    assert [L.smfft_bands_frames(x, 512, 128) for x in (0, 511, 512, 639, 640)] == [0, 0, 1, 1, 2]
    assert L.smfft_bands_frames(-1, 512, 128) == -1 and L.smfft_bands_frames(4096, 512, 0) == -1

    def tables(n, first, count, weights=None, plan_words=None):
        first, count = np.asarray(first, np.int32), np.asarray(count, np.int32)
        total = int(np.maximum(count, 0).sum())
        w = np.arange(1, total + 1, dtype=np.float32) if weights is None else weights
        plan = np.full(3 * first.size + total + 2 if plan_words is None else plan_words, -7, np.int32)
        rc = L.smfft_bands_tables(n, first.size, first.ctypes.data, count.ctypes.data, None if w is None or not w.size else w.ctypes.data, plan.ctypes.data)
        return rc, plan
    for n in (512, 8192):
        M = n // 2
        rc, plan = tables(n, [3, 0, M, 0, 7], [4, 1, 1, M + 1, 0])
        B, nw = 5, M + 7
        assert rc == 0 and plan[:B].tolist() == [3, 0, M, 0, 7] and plan[B:2 * B].tolist() == [4, 1, 1, M + 1, 0]
        assert plan[2 * B:3 * B].tolist() == [0, 4, 5, 6, M + 7] and np.array_equal(plan[3 * B:3 * B + nw].view(np.float32), np.arange(1, nw + 1, dtype=np.float32))
        assert plan[3 * B + nw:].tolist() == [-7, -7], "the plan is plan_bytes long and no longer"
        assert L.smfft_bands_plan_bytes(n, B, nw) == 4 * (3 * B + nw)
        # at the boundaries: a band that ends with bin M, an empty band at first = M + 1, M + 1 bands, exactly 4 (M + 1) weights
        assert tables(n, [M], [1])[0] == 0 and tables(n, [M + 1], [0])[0] == 0 and tables(n, [0], [M + 1])[0] == 0
        assert tables(n, np.arange(M + 1), np.ones(M + 1, int))[0] == 0
        assert tables(n, [0, 0, 0, 0], [M + 1] * 4)[0] == 0
        assert tables(n, [0, 5], [0, 0], np.zeros(0, np.float32))[0] == 0                       # no weights at all: h_weights may be NULL
        # one past them
        untouched = np.full(64, -7, np.int32)
        for first, count in (([M], [2]), ([M + 1], [1]), ([M + 2], [0]), ([0], [M + 2]), ([-1], [1]), ([3], [-1]), ([0, 0, 0, 0, 0], [M + 1] * 4 + [1]),
                             ([2 ** 31 - 1], [2 ** 31 - 1]), ([1], [2 ** 31 - 1])):
            rc, plan = tables(n, first, count, np.zeros(1, np.float32), 64)
            assert rc == -1 and np.array_equal(plan, untouched), (n, first, count)
        assert tables(n, np.zeros(M + 2, int), np.zeros(M + 2, int), np.zeros(0, np.float32))[0] == -1      # more than M + 1 bands
        one = np.zeros(1, np.int32)
        assert L.smfft_bands_tables(n, 0, one.ctypes.data, one.ctypes.data, None, untouched.ctypes.data) == -1
        assert L.smfft_bands_tables(n, 1, None, one.ctypes.data, None, untouched.ctypes.data) == -1
        assert L.smfft_bands_tables(n, 1, one.ctypes.data, None, None, untouched.ctypes.data) == -1
        assert L.smfft_bands_tables(n, 1, one.ctypes.data, one.ctypes.data, None, None) == -1
        three = np.array([3], np.int32)
        assert L.smfft_bands_tables(n, 1, one.ctypes.data, three.ctypes.data, None, untouched.ctypes.data) == -1     # weights, but no array of them
    assert L.smfft_bands_tables(500, 1, one.ctypes.data, one.ctypes.data, None, untouched.ctypes.data) == -1
    # the mirror: the same plan as bytes, ValueError for what the library refuses
    plan = bd.tables(512, [3, 9], [2, 0], [0.5, -1.0])
    assert plan.dtype == np.uint8 and plan.view(np.int32)[:6].tolist() == [3, 9, 2, 0, 0, 2] and plan.view(np.float32)[6:].tolist() == [0.5, -1.0]
    for first, count, w in (([256], [2], [1, 1]), ([0], [1], [1, 2]), ([0, 1], [1], [1]), ([-1], [1], [1]), ([0], [-1], [])):
        with pytest.raises(ValueError):
            bd.tables(512, first, count, w)
    with pytest.raises(ValueError):
        bd.plan_bytes(512, 258, 0)
    assert bd.plan_bytes(8192, 128, 8098) == 12 * 128 + 4 * 8098


# ---- 5: rejections -------------------------------------------------------------------------------------------------
def test_unsupported_combinations_return_minus_one_without_a_device(bands_lib):
    """-1 (or 0 for a zero count) before any HIP call: run in a process where no GPU is visible, with addresses that are never read.
    Every n next to the five, bands 0 and M + 2, weights -1 and 4 (M + 1) + 1, a NULL plan, negative counts, hop 0, stream_stride 0,
    counts beyond 2^59, grid 0, the output starting inside the signal's extent, at its last float, on the window and on the plan --
    its first and its last word -- and smfft_bands_prepare's refusals, which come before its copy"""
    code = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
ll, d, vp, i = ctypes.c_longlong, ctypes.c_double, ctypes.c_void_p, ctypes.c_int
B = [vp, vp, vp, vp, i, i, i, ll, ll, ll, ll]
lib.smfft_bands_launch.argtypes = B + [vp]
lib.smfft_bands_launch_tuned.argtypes = B + [vp, i]
lib.smfft_bands_benchmark.argtypes = B + [ctypes.POINTER(d)]
lib.smfft_bands_prepare.argtypes = [i, i, vp, vp, vp, vp, vp]
t = d(0.0)
IN, OUT, WIN, PLAN = 1 << 30, 1 << 40, 1 << 20, 1 << 36
def forms(n, bands, weights, streams, frames, hop, stride, grid=3, din=IN, dout=OUT, win=WIN, plan=PLAN):
    a = (din, dout, win, plan, n, bands, weights, streams, frames, hop, stride)
    return [lib.smfft_bands_launch(*a, None), lib.smfft_bands_launch_tuned(*a, None, grid), lib.smfft_bands_benchmark(*a, ctypes.byref(t))]
rc, empty = [], []
for n in (256, 500, 16384, 0, -512, 511, 513, 1000, 1023, 1025, 2047, 2049, 4095, 4097, 8191, 8193, 2**31 - 1):
    rc += forms(n, 40, 500, 2, 5, 128, 65536) + forms(n, 40, 500, 0, 0, 128, 65536)
for n in (512, 8192):
    M, hop, S = n // 2, n // 4, 20 * n
    for bands, weights in ((0, 0), (-1, 10), (M + 2, 10), (40, -1), (40, 4 * (M + 1) + 1)):
        rc += forms(n, bands, weights, 2, 5, hop, S) + forms(n, bands, weights, 0, 5, hop, S)
    empty += forms(n, 1, 0, 0, 5, hop, S) + forms(n, M + 1, 4 * (M + 1), 2, 0, hop, S)          # at the boundaries, nothing to do
    rc += forms(n, 40, 500, 2, 5, hop, S, plan=None) + forms(n, 40, 500, 0, 5, hop, S, plan=None)
    rc += forms(n, 40, 500, -1, 5, hop, S) + forms(n, 40, 500, 2, -1, hop, S) + forms(n, 40, 500, -1, 0, hop, S) + forms(n, 40, 500, 0, -1, hop, S)
    rc += forms(n, 40, 500, 2, 5, 0, S) + forms(n, 40, 500, 2, 5, -hop, S) + forms(n, 40, 500, 2, 5, hop, 0) + forms(n, 40, 500, 2, 5, hop, -1)
    rc += forms(n, 40, 500, 0, 5, 0, S) + forms(n, 40, 500, 2, 0, hop, 0)
    rc += forms(n, 40, 500, 2**40, 2**40, hop, S) + forms(n, 40, 500, 2, 2**62, hop, S) + forms(n, 40, 500, 2, 5, 2**62, S) + forms(n, 40, 500, 2, 5, hop, 2**62)
    # 2 streams of 5 frames at hop n / 4, stride 20 n: the extent is 20 n + 4 hop + n floats, the output 10 * 40 floats, the plan
    # 3 * 40 + 500 words
    extent, outs, words = S + 4 * hop + n, 400, 620
    for off in (0, 4, 4 * (extent - 1), -4, -4 * (outs - 1)):
        rc += forms(n, 40, 500, 2, 5, hop, S, dout=IN + off)
    for off in (0, 4 * (outs - 1), -4 * (n - 1)):
        rc += forms(n, 40, 500, 2, 5, hop, S, win=OUT + off)
    for off in (0, 4 * (outs - 1), -4 * (words - 1)):
        rc += forms(n, 40, 500, 2, 5, hop, S, plan=OUT + off)
    # ... and next to them: the output right behind the extent, the window and the plan right behind the output and right in front of it
    empty += [lib.smfft_bands_launch(IN, IN + 4 * extent, WIN, PLAN, n, 40, 500, 0, 5, hop, S, None)]
    for grid in (0, -1):
        rc += [lib.smfft_bands_launch_tuned(IN, OUT, WIN, PLAN, n, 40, 500, streams, 5, hop, S, None, grid) for streams in (2, 0)]
    # prepare: the table is checked before anything is copied
    one, two = (ctypes.c_int * 1)(M), (ctypes.c_int * 1)(2)
    w = (ctypes.c_float * 2)(1.0, 1.0)
    rc += [lib.smfft_bands_prepare(n, 1, one, two, w, PLAN, None), lib.smfft_bands_prepare(n, 0, one, two, w, PLAN, None),
           lib.smfft_bands_prepare(n, 1, one, (ctypes.c_int * 1)(1), w, None, None), lib.smfft_bands_prepare(500, 1, one, two, w, PLAN, None)]
for n in (512, 1024, 2048, 4096, 8192):
    empty += forms(n, 40, 500, 0, 5, n // 4, 6 * n) + forms(n, 40, 500, 2, 0, n // 4, 6 * n) + forms(n, 1, 0, 0, 0, 1, 1, dout=IN, win=None)
print(len(rc), [r for r in rc if r != -1], [e for e in empty if e != 0], t.value)
sys.exit(0 if rc and rc == [-1] * len(rc) and empty and empty == [0] * len(empty) and t.value == 0.0 else 1)
"""
    p = subprocess.run([sys.executable, "-c", code, bands_lib], capture_output=True, text=True, timeout=120, env=dict(os.environ, **NO_DEVICE))
    assert p.returncode == 0, p.stdout + p.stderr


def test_python_wrappers_refuse_before_a_device(bands_lib):
    """in a process where no GPU is visible: the pointer forms turn the library's -1 into a RuntimeError, the table and tensor forms
    raise ValueError or TypeError themselves -- float64, wrong ranks, non-contiguous tensors, windows of another length, an out of
    another shape, something that is no Plan, tensors on the host -- and a zero count is served"""
    code = ac.REFUSED + r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from smfft_amd import bands
IN, OUT, WIN, PLAN = 1 << 30, 1 << 40, 1 << 20, 1 << 36
for n in (256, 500, 16384, 0):
    refused(RuntimeError, bands.launch_ptr, IN, OUT, WIN, PLAN, n, 40, 500, 2, 5, 128, 65536)
    refused(RuntimeError, bands.launch_ptr, IN, OUT, WIN, PLAN, n, 40, 500, 2, 5, 128, 65536, grid=3)
    assert bands.benchmark(IN, OUT, WIN, PLAN, n, 40, 500, 2, 5, 128, 65536) == (-1, 0.0)
    refused(ValueError, bands.fft_size, n)
    refused(ValueError, bands.frames, 1 << 20, n, 128)
    refused(ValueError, bands.plan_bytes, n, 40, 500)
    refused(ValueError, bands.tables, n, [0], [1], [1.0])
    refused(ValueError, bands.prepare, n, [0], [1], [1.0], "cpu")
    refused(ValueError, bands.prepare_ptr, n, [0], [1], [1.0], PLAN)
    refused(ValueError, bands.mel_filterbank, n, 16000, 40)
    refused(ValueError, bands.uniform_bands, n, 4)
refused(RuntimeError, bands.launch_ptr, IN, OUT, WIN, PLAN, 512, 0, 0, 2, 5, 128, 65536)
refused(RuntimeError, bands.launch_ptr, IN, OUT, WIN, PLAN, 512, 258, 0, 2, 5, 128, 65536)
refused(RuntimeError, bands.launch_ptr, IN, OUT, WIN, PLAN, 512, 40, 1029, 2, 5, 128, 65536)
refused(RuntimeError, bands.launch_ptr, IN, OUT, WIN, PLAN, 512, 40, 500, 2, 5, 0, 65536)
refused(RuntimeError, bands.launch_ptr, IN, OUT, WIN, PLAN, 512, 40, 500, 2, 5, 128, 65536, grid=0)
refused(RuntimeError, bands.launch_ptr, IN, IN + 4, WIN, PLAN, 512, 40, 500, 2, 5, 128, 65536)
refused(RuntimeError, bands.launch_ptr, IN, OUT, WIN, OUT + 4, 512, 40, 500, 2, 5, 128, 65536)
refused(RuntimeError, bands.launch_ptr, IN, OUT, OUT, PLAN, 512, 40, 500, 2, 5, 128, 65536)
refused(RuntimeError, bands.launch_ptr, IN, OUT, WIN, None, 512, 40, 500, 2, 5, 128, 65536)
refused(ValueError, bands.prepare_ptr, 512, [256], [2], [1.0, 1.0], PLAN)
refused(ValueError, bands.prepare, 512, [0, 0, 0, 0, 0], [257, 257, 257, 257, 1], np.ones(1029), "cpu")
assert [bands.frames(L, 512, 128) for L in (0, 511, 512, 639, 640)] == [0, 0, 1, 1, 2] and bands.fft_size(8192) == 4096
import torch
plan = bands.prepare(512, *bands.uniform_bands(512, 4), device="cpu")
assert plan.bands == 65 and plan.weights == 257 and plan.n == 512 and plan.tensor.dtype == torch.uint8 and plan.tensor.numel() == 12 * 65 + 4 * 257
assert plan.dense().shape == (65, 257) and plan.dense().sum() == 257
sig = torch.zeros(2, 4096)
for f in (lambda s, *a, **k: bands.band_spectrogram(s, plan, 128, *a, **k), lambda s, *a, **k: bands.launch(s, None, plan, 128, *a, **k),
          lambda s, *a, **k: bands.mel_spectrogram(s, 16000, 512, 128, 40, window=(a[0] if a else None), **k)):
    refused(TypeError, f, np.zeros((2, 4096), np.float32))
    refused(TypeError, f, sig.double())
    refused(ValueError, f, torch.zeros(2, 2, 4096))                       # three axes
    refused(ValueError, f, torch.zeros(2, 500))                           # shorter than a frame
    refused(ValueError, f, torch.zeros(2, 8192)[:, ::2])                  # not contiguous
    refused(ValueError, f, sig, torch.zeros(256))                         # a window of another length
    refused(TypeError, f, sig, torch.zeros(512, dtype=torch.float64))
    refused(ValueError, f, sig)                                           # a tensor on the host: no CPU fallback
refused(ValueError, bands.band_spectrogram, sig, plan, 0)
refused(TypeError, bands.band_spectrogram, sig, plan.tensor, 128)
refused(TypeError, bands.launch, sig, None, (plan.first, plan.count, plan.w), 128)
refused(ValueError, bands.launch, sig, torch.zeros(2, 29, 64), plan, 128)                 # 65 bands, not 64
refused(TypeError, bands.launch, sig, torch.zeros(2, 29, 65, dtype=torch.float64), plan, 128)
refused(ValueError, bands.band_spectrogram, torch.zeros(2, 200), plan, 128, center=True)
refused(ValueError, bands.mel_spectrogram, sig, 16000, 500, 128, 40)
refused(ValueError, bands.mel_spectrogram, sig, 16000, 512, 128, 40, log="log2")
refused(ValueError, bands.mel_spectrogram, sig, 16000, 512, 128, 40, mel_scale="bark")
refused(ValueError, bands.mel_spectrogram, sig, 16000, 512, 128, 0)
bands.launch_ptr(IN, OUT, None, PLAN, 512, 40, 500, 0, 5, 128, 65536)                     # an empty batch: nothing is launched
bands.launch_ptr(IN, OUT, None, PLAN, 8192, 40, 500, 2, 0, 128, 65536, grid=2)
assert bands.benchmark(IN, OUT, None, PLAN, 512, 40, 500, 2, 0, 128, 65536) == (0, 0.0)
print("ok")
"""
    p = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300, env=dict(os.environ, **NO_DEVICE))
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout + p.stderr


def test_import_does_not_load_the_library():
    ac.check_import_does_not_load("bands", "smfft_bands")

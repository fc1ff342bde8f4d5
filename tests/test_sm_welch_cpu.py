"""CPU checks of the Welch library (smfft_amd/csrc/smfft_welch.hip, libsmfft_welch.so): the model (tools/welch_model.py on
tools/stft_model.py) in fp64 is the sums of the definition and, through the scaling of smfft_amd.welch, scipy.signal.welch / csd /
coherence with detrend=False, and in fp32 -- sequential sums in frame order -- it stays inside the GPU tests' bounds; the gfx950 code
of the ten kernels keeps its budget; and the C ABI declares, exports and validates the eight entry points without a device.  No GPU
code is run (hipcc cross-compiles gfx950)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import stft_model as sm  # noqa: E402
import welch_model as wm  # noqa: E402

from tests import addon_checks as ac  # noqa: E402
from tests import welch_inventory  # noqa: E402
from tests.fir_gpu_harness import ROW_MAX, ROW_REL_L2  # noqa: E402

CSRC = ac.CSRC
LIB = os.path.join(ROOT, "smfft_amd", "libsmfft_welch.so")
SIZES = (256, 512, 1024, 2048, 4096)
LENGTHS = (512, 1024, 2048, 4096, 8192)
FORMS = ("launch", "launch_tuned", "benchmark")
NAMES = ("smfft_welch_fft_size", "smfft_welch_groups") + tuple(f"smfft_{t}_{f}" for t in ("welch", "csd") for f in FORMS)
LDS_BUDGET = 34816             # 4096 / 16 * 17 float2: the transform region of 4096 points
LDS_WITH_SUMS = 34816 + 32768  # ... and sixteen complex sums of 256 threads behind it: the cross kernel from M = 512 on
NO_DEVICE = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


@pytest.fixture(scope="module")
def welch_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", CSRC, "-j", "4", "../libsmfft_welch.so"])
    return LIB


def _pair(rng, shape):
    """x and y = 0.7 (x delayed by 3) + 0.5 noise, float32"""
    x = rng.standard_normal(shape).astype(np.float32)
    y = (0.5 * rng.standard_normal(shape)).astype(np.float32)
    y[..., 3:] += np.float32(0.7) * x[..., :-3]
    return x, y


# ---- 1: the model -------------------------------------------------------------------------------------------
def test_fp64_model_is_the_direct_sums():
    """n = 512, 2 streams of 7 frames in groups of 3 (the seventh frame is left out), with a window that has no symmetry and without
    one: the auto and cross sums of the fp64 chain within 1e-12 of the sums of the definition; the cross spectrum of a signal with
    itself is its auto spectrum; the imaginary parts of bins 0 and M are zero"""
    n, hop, T = 512, 129, 3
    x, y = _pair(np.random.default_rng(270), (2, 6 * hop + n))
    fx, fy = sm.frames(x, n, hop), sm.frames(y, n, hop)
    assert fx.shape == (2, 7, n)
    ramp = sm.hann(n) * (1 + np.arange(n) / (2 * n)) + 0.1
    for win in (None, sm.hann(n), ramp):
        got, want = wm.auto(fx, T, win), wm.direct_auto(fx, T, win)
        assert got.shape == (2, 2, n // 2 + 1) and got.dtype == np.float64
        l2, mx = wm.errors(got, want)
        assert l2.max() <= 1e-12 and mx.max() <= 1e-12, (l2.max(), mx.max())
        got, want = wm.cross(fx, fy, T, win), wm.direct_cross(fx, fy, T, win)
        assert got.shape == (2, 2, n // 2 + 1) and got.dtype == np.complex128
        l2, mx = wm.errors(got, want)
        print(f"fp64 model against the direct sums: relL2 = {l2.max():.2e}, max = {mx.max():.2e}")
        assert l2.max() <= 1e-12 and mx.max() <= 1e-12, (l2.max(), mx.max())
        assert np.all(got[..., 0].imag == 0) and np.all(got[..., -1].imag == 0)
        same = wm.cross(fx, fx, T, win)
        l2, mx = wm.errors(same, wm.auto(fx, T, win))
        assert l2.max() <= 1e-14 and mx.max() <= 1e-14
    p = np.arange(24, dtype=np.float32).reshape(1, 6, 4)
    assert np.array_equal(wm.sequential_sum(p, 3), np.stack([p[:, 0] + p[:, 1] + p[:, 2], p[:, 3] + p[:, 4] + p[:, 5]], axis=1))
    assert np.array_equal(wm.sequential_sum(p, 1), p)


@pytest.mark.parametrize("scaling", ["density", "spectrum"])
def test_fp64_model_is_scipys(scaling):
    """scipy.signal.welch / csd / coherence with detrend=False, return_onesided=True, an odd hop and a frame count that is no multiple
    of anything: the sum over all frames of the fp64 model times welch_model.scale -- the factors smfft_amd.welch applies -- within
    1e-12 of scipy's, with the periodic Hann window and the boxcar, fs = 1 and 3"""
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(271)
    for n, hop, F in ((512, 129, 11), (2048, 512, 5)):
        x, y = _pair(rng, (2, (F - 1) * hop + n + 7))
        x, y = x.astype(np.float64), y.astype(np.float64)
        fx, fy = sm.frames(x, n, hop), sm.frames(y, n, hop)
        assert fx.shape[1] == F
        for w, fs in ((sm.hann(n), 1.0), (np.ones(n), 3.0)):
            kw = dict(fs=fs, window=w, nperseg=n, noverlap=n - hop, detrend=False, return_onesided=True, scaling=scaling)
            s = wm.scale(n, F, w, fs, scaling)
            pxx, pyy, pxy = wm.auto(fx, F, w)[:, 0], wm.auto(fy, F, w)[:, 0], wm.cross(fx, fy, F, w)[:, 0]
            for got, want in ((pxx * s, signal.welch(x, **kw)[1]), (pxy * s, signal.csd(x, y, **kw)[1])):
                l2, mx = wm.errors(got, want)
                print(f"n={n} {scaling}: against scipy relL2 = {l2.max():.2e}, max = {mx.max():.2e}")
                assert l2.max() <= 1e-12 and mx.max() <= 1e-12, (n, scaling, l2.max(), mx.max())
            kw.pop("scaling"), kw.pop("return_onesided")
            want = signal.coherence(x, y, **kw)[1]
            assert np.max(np.abs(wm.coherence(pxx, pyy, pxy) - want)) <= 1e-12
    with pytest.raises(ValueError):
        wm.scale(512, 3, None, 1.0, "power")


def test_python_scaling_is_the_models():
    """smfft_amd.welch._scale, the factors of welch() and csd(), are welch_model.scale's, on the host"""
    import torch
    from smfft_amd import welch
    for n, F, fs in ((512, 11, 1.0), (8192, 3, 48000.0)):
        for w in (None, torch.from_numpy(sm.hann(n, np.float32))):
            for scaling in ("density", "spectrum"):
                got = welch._scale(n, F, w, fs, scaling, "cpu").numpy()
                want = wm.scale(n, F, None if w is None else w.numpy().astype(np.float64), fs, scaling)
                assert got.shape == (n // 2 + 1,) and np.max(np.abs(got / want - 1)) <= 1e-14
    # default_T: the largest T that leaves streams * groups >= 16 * 256 * 2 * slots per workgroup, at least 1
    assert welch.default_T(64, 65533, 512) == 65533 // -(-16 * 256 * 2 * 16 // 64) == 31
    assert welch.default_T(64, 1024, 8192) == 8 and welch.default_T(1, 100, 8192) == 1 and welch.default_T(4096, 100, 8192) == 50


def test_fp32_model_is_inside_the_bounds():
    """every stage of the chain rounded to fp32 and the sums sequential in fp32, n = 512 and 8192, T = 3, 7 and 64: the auto spectra
    against themselves in fp64 and the cross spectra against sqrt(Pxx Pyy) inside 2 ROW_REL_L2 + (T - 1) 2^-24 and
    2 ROW_MAX + (T - 1) 2^-24, the bounds of the GPU tests"""
    worst = {}
    for n, T in ((512, 3), (512, 7), (512, 64), (8192, 3)):
        rng = np.random.default_rng(272 + n + T)
        hop = n // 4 + 1
        x, y = _pair(rng, (2, (T - 1) * hop + n))
        fx, fy = sm.frames(x, n, hop), sm.frames(y, n, hop)
        for name, w in (("hann", sm.hann(n, np.float32)), ("no window", None)):
            pxx, pyy = wm.auto(fx, T, w), wm.auto(fy, T, w)
            cases = {"auto": (wm.auto(fx, T, w, np.float32), pxx, None), "cross": (wm.cross(fx, fy, T, w, np.float32), wm.cross(fx, fy, T, w), np.sqrt(pxx * pyy))}
            for kind, (got, want, norm) in cases.items():
                assert got.dtype == (np.float32 if kind == "auto" else np.complex64)
                l2, mx = wm.errors(got, want, norm)
                print(f"n={n} T={T} {kind}, {name}: fp32 model relL2 = {l2.max():.2e}, max = {mx.max():.2e}")
                key = (kind, T > 7)
                worst[key] = [max(a, b) for a, b in zip(worst.get(key, [0.0, 0.0]), (l2.max(), mx.max()))]
                assert l2.max() <= 2 * ROW_REL_L2 + (T - 1) * 2.0 ** -24 and mx.max() <= 2 * ROW_MAX + (T - 1) * 2.0 ** -24, (n, T, kind, name)
    for (kind, long), (l2, mx) in worst.items():
        print(f"fp32 model, worst {kind} at T {'= 64' if long else '<= 7'}: relL2 = {l2:.2e}, max |d| / max ref = {mx:.2e}")
    assert ROW_REL_L2 == 1e-6 and ROW_MAX == 5e-6


def test_source_repeats_the_stft_step_and_builds_on_the_shared_layers():
    """the frame-to-spectrum statements of smfft_stft.hip stand in smfft_welch.hip as they are (DESIGN.md section 27 says why they are
    written twice); the twiddle row comes from the shared table; the sample loads go through rows::gload2; the entry points are the
    shared host layer's; nothing transcendental"""
    source, stft = open(os.path.join(CSRC, "smfft_welch.hip")).read(), open(os.path.join(CSRC, "smfft_stft.hip")).read()
    for line in ("fwd.transform(r, sf);", "for (int q = 0; q < 16; ++q) sf[fwd.u + T * q] = r[q];", "const float2* partner = sf + (T - fwd.u);",
                 "for (int q = 0; q < 16; ++q) p[q] = partner[T * (15 - q)];", "p[0] = self ? r[0] : p[0];", "const int u = per_tile(fwd.u);",
                 "const float2 w = row_entry(&rows<M>.wn[u + T * q]);",
                 "const float sx = r[q].x + p[q].x, sy = r[q].y - p[q].y, dx = r[q].x - p[q].x, dy = r[q].y + p[q].y;",
                 "r[q] = make_float2(0.5f * (sx - w.y * dx + w.x * dy), 0.5f * (sy - w.y * dy - w.x * dx));",
                 "r[0] = self ? make_float2(x0, 0.f) : r[0];", "const float pw = r[q].x * r[q].x + r[q].y * r[q].y;",
                 "const float v0 = r[q].x * w[q].x;", "const float v1 = r[q].y * w[q].y;", "wn[k] = w32768(k * (16384 / M))"):
        assert line in source and line in stft, line
    assert '#include "smfft_rows.hpp"' in source and '#include "smfft_rows_host.hpp"' in source and not re.search(r'#include "[^"]*\.inc"', source)
    assert "rows::gload2<SMFFT_WELCH_NT_LOAD != 0>" in source
    for f in ("checked_launch(", "checked_launch_tuned(", "checked_benchmark("):
        assert source.count(f) == 2, f
    assert not re.search(r"\b(sinf?|cosf?|sincosf?|__sinf|__cosf)\s*\(", re.sub(r"//[^\n]*", "", source))
    assert "const float re = xs[q].x * r[q].x + xs[q].y * r[q].y;" in source and "const float im = a - b;" in source
    assert "atomic" not in source.lower() and "hipMalloc" not in source
    assert "## 27. Welch power and cross spectra" in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---- 2: ISA budget and inventory -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """{M: assembly of smfft_welch_<M>.o as the Makefile compiles it}"""
    if not os.path.exists(ac.HIPCC):
        pytest.skip("hipcc not installed")
    return ac.addon_isa("smfft_welch", "WELCH", SIZES, tmp_path_factory.mktemp("welch_isa"))


def test_isa_budget_of_what_ships(isa):
    """per M exactly the two kernels, read from the compiled object's metadata: no scratch, at most 256 VGPRs (two waves per SIMD),
    static LDS of exactly 34,816 B for welch_kernel and for csd_kernel at M = 256, and 67,584 B -- the sums of the cross spectrum behind
    the transform region, two workgroups per compute unit -- for csd_kernel from M = 512 on; no transcendentals; 17 non-temporal
    stores, 4 bytes each (welch) or 8 (csd), behind every global load"""
    total = 0
    for m, text in isa.items():
        descs = ac.descriptors(text)
        kernels = {}
        for family in ("welch", "csd"):
            found = ac.pfb_kernels(text, r"\d+%s_kernel" % family)
            assert len(found) == 1, (m, family, sorted(found))
            kernels.update({name: (family, body) for name, body in found.items()})
        assert len(descs) == 2 and set(descs) == set(kernels), (m, sorted(descs))
        total += len(descs)
        assert not re.search(r"\bscratch_", text), m
        for name, (family, body) in kernels.items():
            assert re.search(r"%s_kernelILi%dE" % (family, m), name)
            assert not [line for line in body if re.match(r"v_(sin|cos)_", line)], name
            assert ac.descriptor_field(descs, name, "private_segment_fixed_size") == 0, name
            v, lds = ac.descriptor_field(descs, name, "next_free_vgpr"), ac.descriptor_field(descs, name, "group_segment_fixed_size")
            print(f"M={m}: {family}_kernel: {v} VGPRs ({ac.occupancy(v)} waves per SIMD), {lds} B of LDS, 0 B of scratch")
            assert lds == (LDS_WITH_SUMS if family == "csd" and m > 256 else LDS_BUDGET) and 2 * lds <= ac.LDS_PER_CU, (name, lds)
            assert v <= 256 and ac.occupancy(v) >= 2, (name, v)
            loads = [i for i, line in enumerate(body) if line.startswith("global_load")]
            stores = [i for i, line in enumerate(body) if line.startswith("global_store")]
            assert not [i for i in loads if re.search(r"\bnt\b", body[i])], name           # the shipped policy: plain sample loads
            assert len(loads) >= 48, (name, len(loads))                                      # samples, window, W_n (the cross kernel: twice)
            assert len(stores) == 17, (name, len(stores))
            width = r"global_store_dword\s" if family == "welch" else r"global_store_dwordx2\s"
            assert all(re.match(width, body[i]) and re.search(r"\bnt\b", body[i]) for i in stores), name
            assert min(stores) > max(loads), name
    assert total == 10


def test_library_ships_ten_kernels_and_the_inventory_names_them(welch_lib):
    ac.check_inventory(welch_lib, welch_inventory.KERNELS, "smfft_", 10, kinds=("tests", "bounds", "probes"))
    assert len(welch_inventory.KERNELS) == 10
    for family in welch_inventory.FAMILIES:
        assert all(e["call"].startswith(f"smfft_{family}_launch") for k, e in welch_inventory.KERNELS.items() if f"::{family}_kernel<" in k)
    assert "permlane" in welch_inventory.__doc__ and "hostsim" in welch_inventory.__doc__ and "stft_inventory" in welch_inventory.__doc__


def test_isa_identity_compares_the_library():
    """tools/isa_identity.py compiles the five objects with the Makefile's flags and -I., like the other add-ons' (the tool itself
    needs the history of a git checkout and minutes of compiling: it is run by hand, DESIGN.md section 27 has its verdict)"""
    ac.check_isa_identity_lists("smfft_welch", "WELCH", SIZES)
    assert all("-ffp-contract=on" in ac.makefile_flags("WELCH", m) for m in SIZES)


# ---- 3: declarations and exports ---------------------------------------------------------------------------------
def test_python_mirror_matches_header(welch_lib):
    from smfft_amd import welch
    header = re.sub(r"[\s*]+", " ", open(os.path.join(ROOT, "include", "smfft_welch.h")).read())
    for phrase in ("S[(c groups + g) (M + 1) + k] = sum_{t<T} p[c, g T + t, k]", "C[(c groups + g) (M + 1) + k] = sum_{t<T} conj(X[c, g T + t, k]) Y[c, g T + t, k]",
                   "scipy.signal.csd's convention", "re = xr yr + xi yi in one expression", "im = a - b with a = xr yi and b = xi yr",
                   "acc = p_0, then acc += p_t", "With T = 1 the auto spectra equal smfft_stft_launch(kind = 1) bit for bit",
                   "The real part of csd(x, x) equals the auto spectrum to the bit and its imaginary part is exactly +0",
                   "The imaginary parts of bins 0 and M are stored as exactly +0", "NULL means all ones",
                   "No plan, no table to prepare, no workspace, no atomics and no allocation in a call",
                   "every output element is written exactly once", "frames f >= groups T are never read",
                   "y_stride = 0 is allowed and means one reference stream for all c", "d_x == d_y is legal",
                   "The output may overlap neither the extent of x, nor that of y, nor the window", "allocate nothing and do not synchronise",
                   "A NaN or Inf stays in the groups whose frames contain the sample", "T < 1", "x_stride < 1 or y_stride < 0",
                   "beyond 2^59 elements (computed in 128 bits)", "grid < 1 (launch_tuned)", "a forbidden overlap",
                   "A zero count launches nothing and returns 0", "Out of scope", "detrend='constant'", "median averaging", "two-sided output",
                   "n < 512", "not a power of two", "a fused Pxx / Pyy / Pxy kernel for coherence", "compensated or fp64 accumulation",
                   "cross spectra of all pairs of streams (a correlator)"):
        assert re.sub(r"[\s*]+", " ", phrase) in header, phrase
    decl = ac.declarations("smfft_welch.h")
    assert sorted(decl) == sorted(welch.SIGS) == sorted(NAMES)
    for name, (res, args) in decl.items():
        assert welch.SIGS[name] == ac.signature(res, args), name
    assert welch.SIZES == SIZES and welch.LENGTHS == LENGTHS
    for f in ("welch", "csd", "coherence", "dynamic_spectrum", "launch", "csd_launch", "launch_ptr", "csd_ptr", "welch_benchmark", "csd_benchmark",
              "groups", "fft_size", "default_T", "hann"):
        assert callable(getattr(welch, f)), f


def test_library_exports_exactly_the_eight_symbols(welch_lib):
    ac.check_exports(welch_lib, NAMES)
    assert len(NAMES) == 8


# ---- 4: rejections -------------------------------------------------------------------------------------------------
def test_unsupported_combinations_return_minus_one_without_a_device(welch_lib):
    """-1 (or 0 for a zero count) before any HIP call: run in a process where no GPU is visible, with addresses that are never read.
    Every n next to the five, T 0 and negative, negative counts, hop 0, x_stride 0, y_stride -1 (y_stride 0 is served: with zero
    groups it returns 0, and it is refused only for its overlap), counts beyond 2^59, grid 0, the output starting inside x's extent,
    inside y's, at their last floats and on the window; and smfft_welch_groups"""
    code = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
ll, d, vp, i = ctypes.c_longlong, ctypes.c_double, ctypes.c_void_p, ctypes.c_int
dp = ctypes.POINTER(d)
W, X = [vp, vp, vp, i, ll, ll, ll, ll, ll], [vp, vp, vp, vp, i, ll, ll, ll, ll, ll, ll]
for name, head in (("welch", W), ("csd", X)):
    getattr(lib, f"smfft_{name}_launch").argtypes = head + [vp]
    getattr(lib, f"smfft_{name}_launch_tuned").argtypes = head + [vp, i]
    getattr(lib, f"smfft_{name}_benchmark").argtypes = head + [dp]
lib.smfft_welch_groups.restype, lib.smfft_welch_groups.argtypes = ll, [ll, i, ll, ll]
t = d(0.0)
IN, Y, OUT, WIN = 1 << 30, 1 << 34, 1 << 40, 1 << 20
def forms(name, args, grid=3):
    return [getattr(lib, f"smfft_{name}_launch")(*args, None), getattr(lib, f"smfft_{name}_launch_tuned")(*args, None, grid),
            getattr(lib, f"smfft_{name}_benchmark")(*args, ctypes.byref(t))]
def welch(n, streams, groups, T, hop, stride, grid=3, din=IN, dout=OUT, win=WIN):
    return forms("welch", (din, dout, win, n, streams, groups, T, hop, stride), grid)
def csd(n, streams, groups, T, hop, xs, ys, grid=3, dx=IN, dy=Y, dout=OUT, win=WIN):
    return forms("csd", (dx, dy, dout, win, n, streams, groups, T, hop, xs, ys), grid)
def both(n, streams, groups, T, hop, stride):
    return welch(n, streams, groups, T, hop, stride) + csd(n, streams, groups, T, hop, stride, stride)
rc, ok, groups = [], [], []
for n in (256, 500, 16384, 0, -512, 511, 513, 1000, 1023, 1025, 2047, 2049, 4095, 4097, 8191, 8193, 2**31 - 1):
    rc += both(n, 2, 5, 3, 128, 65536) + both(n, 0, 0, 3, 128, 65536)
    rc += [lib.smfft_welch_fft_size(n), lib.smfft_welch_groups(1 << 20, n, 128, 3)]
for n in (512, 8192):
    hop = n // 4
    S = 20 * n
    for T in (0, -1, -2**40):
        rc += both(n, 2, 5, T, hop, S) + both(n, 0, 5, T, hop, S)
    rc += both(n, -1, 5, 3, hop, S) + both(n, 2, -1, 3, hop, S) + both(n, -1, 0, 3, hop, S) + both(n, 0, -1, 3, hop, S)
    rc += both(n, 2, 5, 3, 0, S) + both(n, 2, 5, 3, -hop, S) + both(n, 2, 5, 3, hop, 0) + both(n, 2, 5, 3, hop, -1) + both(n, 0, 5, 3, 0, S) + both(n, 2, 0, 3, hop, 0)
    rc += csd(n, 2, 5, 3, hop, S, -1) + csd(n, 2, 5, 3, hop, 0, S) + csd(n, 2, 5, 3, hop, 0, 0) + csd(n, 0, 5, 3, hop, S, -1)
    ok += csd(n, 2, 0, 3, hop, S, 0) + csd(n, 0, 5, 3, hop, S, 0)            # y_stride = 0 is a legal argument
    rc += both(n, 2**40, 2**40, 3, hop, S) + both(n, 2, 2**40, 2**40, hop, S) + both(n, 2, 2**62, 2**62, hop, S) + both(n, 2, 5, 3, 2**62, S)
    rc += both(n, 2, 5, 3, hop, 2**62) + csd(n, 2**20, 5, 3, hop, S, 2**60)
    # 2 streams of 5 groups of 3 frames at hop n / 4, stride 20 n: the extent is 20 n + 14 hop + n floats; the output is 10 (n / 2 + 1)
    # floats (welch) or complex values (csd); with y_stride = 0 the extent of y is 14 hop + n
    extent, one = S + 14 * hop + n, 14 * hop + n
    outs = 10 * (n // 2 + 1)
    for off in (0, 4, 4 * (extent - 1), -4, -4 * (outs - 1)):
        rc += welch(n, 2, 5, 3, hop, S, dout=IN + off)
    for off in (0, 4, 4 * (extent - 1), -4, -4 * (2 * outs - 1)):
        rc += csd(n, 2, 5, 3, hop, S, S, dout=IN + off) + csd(n, 2, 5, 3, hop, S, S, dout=Y + off)
    for off in (0, 4 * (one - 1), -4 * (2 * outs - 1)):
        rc += csd(n, 2, 5, 3, hop, S, 0, dout=Y + off)
    ok += [lib.smfft_csd_launch(IN, Y, Y + 4 * one, WIN, n, 0, 5, 3, hop, S, 0, None)]
    for off in (0, 4 * (outs - 1), -4 * (n - 1)):
        rc += welch(n, 2, 5, 3, hop, S, win=OUT + off)
    for off in (0, 4 * (2 * outs - 1), -4 * (n - 1)):
        rc += csd(n, 2, 5, 3, hop, S, S, win=OUT + off)
    for grid in (0, -1):
        rc += [lib.smfft_welch_launch_tuned(IN, OUT, WIN, n, streams, 5, 3, hop, S, None, grid) for streams in (2, 0)]
        rc += [lib.smfft_csd_launch_tuned(IN, Y, OUT, None, n, streams, 5, 3, hop, S, 0, None, grid) for streams in (2, 0)]
    rc += [lib.smfft_welch_groups(-1, n, hop, 3), lib.smfft_welch_groups(1 << 20, n, 0, 3), lib.smfft_welch_groups(1 << 20, n, hop, 0),
           lib.smfft_welch_groups(1 << 20, n, hop, -1)]
    groups += [lib.smfft_welch_groups(L, n, hop, 3) for L in (0, n - 1, n, n + 2 * hop - 1, n + 2 * hop, n + 7 * hop + 1)]
    groups += [lib.smfft_welch_groups(n + 63 * hop, n, hop, T) for T in (1, 64, 65)]
empty = []
for n in (512, 1024, 2048, 4096, 8192):
    empty += both(n, 0, 5, 3, n // 4, 6 * n) + both(n, 2, 0, 3, n // 4, 6 * n) + welch(n, 0, 0, 1, 1, 1, dout=IN, win=None) + csd(n, 0, 0, 1, 1, 1, 0, dout=IN, dy=IN)
sizes = [lib.smfft_welch_fft_size(n) for n in (512, 1024, 2048, 4096, 8192)]
want_groups = [0, 0, 0, 0, 1, 2, 64, 1, 0] * 2
print(len(rc), [r for r in rc if r != -1], [e for e in empty + ok if e != 0], t.value, sizes, groups)
good = rc and rc == [-1] * len(rc) and empty and empty == [0] * len(empty) and ok == [0] * len(ok) and t.value == 0.0
sys.exit(0 if good and sizes == [256, 512, 1024, 2048, 4096] and groups == want_groups else 1)
"""
    p = subprocess.run([sys.executable, "-c", code, welch_lib], capture_output=True, text=True, timeout=120, env=dict(os.environ, **NO_DEVICE))
    assert p.returncode == 0, p.stdout + p.stderr


def test_python_wrappers_refuse_before_a_device(welch_lib):
    """in a process where no GPU is visible: the pointer forms turn the library's -1 into a RuntimeError, the tensor forms raise
    ValueError or TypeError themselves -- float64, wrong ranks, non-contiguous tensors, windows of another length, a y of another
    shape, tensors on the host -- and a zero count is served"""
    code = ac.REFUSED + r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from smfft_amd import welch
IN, Y, OUT, WIN = 1 << 30, 1 << 34, 1 << 40, 1 << 20
for n in (256, 500, 16384, 0):
    refused(RuntimeError, welch.launch_ptr, IN, OUT, WIN, n, 2, 5, 3, 128, 65536)
    refused(RuntimeError, welch.csd_ptr, IN, Y, OUT, WIN, n, 2, 5, 3, 128, 65536, 0, grid=3)
    assert welch.welch_benchmark(IN, OUT, WIN, n, 2, 5, 3, 128, 65536) == (-1, 0.0)
    assert welch.csd_benchmark(IN, Y, OUT, WIN, n, 2, 5, 3, 128, 65536, 65536) == (-1, 0.0)
    refused(ValueError, welch.fft_size, n)
    refused(ValueError, welch.groups, 1 << 20, n, 128, 3)
refused(RuntimeError, welch.launch_ptr, IN, OUT, WIN, 512, 2, 5, 0, 128, 65536)
refused(RuntimeError, welch.launch_ptr, IN, OUT, WIN, 512, 2, 5, 3, 128, 0)
refused(RuntimeError, welch.launch_ptr, IN, OUT, WIN, 512, 2, 5, 3, 128, 65536, grid=0)
refused(RuntimeError, welch.launch_ptr, IN, IN + 4, WIN, 512, 2, 5, 3, 128, 65536)
refused(RuntimeError, welch.csd_ptr, IN, Y, OUT, WIN, 512, 2, 5, 3, 128, 0, 65536)
refused(RuntimeError, welch.csd_ptr, IN, Y, OUT, WIN, 512, 2, 5, 3, 128, 65536, -1)
refused(RuntimeError, welch.csd_ptr, IN, Y, Y + 4, WIN, 512, 2, 5, 3, 128, 65536, 0)
refused(RuntimeError, welch.csd_ptr, IN, Y, OUT, OUT, 512, 2, 5, 3, 128, 65536, 0)
refused(ValueError, welch.groups, 4096, 512, 128, 0)
assert [welch.groups(L, 512, 128, 3) for L in (0, 511, 512, 767, 768)] == [0, 0, 0, 0, 1] and welch.fft_size(8192) == 4096
import torch
sig = torch.zeros(2, 4096)
for f in (lambda s, *a, **k: welch.launch(s, 512, 128, 3, *a, **k), lambda s, *a, **k: welch.dynamic_spectrum(s, 512, 128, 3, *a, **k),
          lambda s, *a, **k: welch.welch(s, 1.0, *a, **k), lambda s, *a, **k: welch.csd(s, s, 1.0, *a, **k),
          lambda s, *a, **k: welch.coherence(s, s, *a, **k), lambda s, *a, **k: welch.csd_launch(s, s, 512, 128, 3, *a, **k)):
    refused(TypeError, f, np.zeros((2, 4096), np.float32))
    refused(TypeError, f, sig.double())
    refused(ValueError, f, torch.zeros(2, 2, 4096))                       # three axes
    refused(ValueError, f, torch.zeros(2, 500))                           # shorter than a frame
    refused(ValueError, f, torch.zeros(2, 8192)[:, ::2])                  # not contiguous
    refused(ValueError, f, sig, torch.zeros(256))                         # a window of another length
    refused(TypeError, f, sig, torch.zeros(512, dtype=torch.float64))
    refused(ValueError, f, sig)                                           # a tensor on the host: no CPU fallback
refused(ValueError, welch.launch, sig, 500, 128, 3)
refused(ValueError, welch.launch, sig, 512, 0, 3)
refused(ValueError, welch.launch, sig, 512, 128, 0)
refused(ValueError, welch.welch, sig, n=500)
refused(ValueError, welch.welch, sig, hop=0)
refused(ValueError, welch.csd, sig, torch.zeros(3, 4096))
refused(ValueError, welch.csd, sig, torch.zeros(2, 4000))
refused(ValueError, welch.coherence, sig, torch.zeros(4096, dtype=torch.float64).float()[:4000])
welch.launch_ptr(IN, OUT, None, 512, 0, 5, 3, 128, 65536)                 # an empty batch: nothing is launched
welch.csd_ptr(IN, Y, OUT, None, 8192, 2, 0, 3, 128, 65536, 0)
assert welch.welch_benchmark(IN, OUT, None, 512, 2, 0, 3, 128, 65536) == (0, 0.0)
print("ok")
"""
    p = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300, env=dict(os.environ, **NO_DEVICE))
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout + p.stderr


def test_import_does_not_load_the_library():
    ac.check_import_does_not_load("welch", "smfft_welch")

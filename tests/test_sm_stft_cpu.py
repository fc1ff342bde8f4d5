"""CPU checks of the STFT library (smfft_amd/csrc/smfft_stft.hip, libsmfft_stft.so): the model's chain (tools/stft_model.py) in fp64 is
the fp64 sum of the definition, np.fft.rfft / irfft and torch.stft / torch.istft, the periodic Hann window at hop n / 4 overlap-adds
to 1.5 and reconstructs the signal, and in fp32 the chain stays inside the GPU tests' bounds; the gfx950 code of the fifteen kernels
keeps its budget; and the C ABI declares, exports and validates the eight entry points without a device.  No GPU code is run (hipcc
cross-compiles gfx950)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import stft_model as sm  # noqa: E402

from tests import addon_checks as ac  # noqa: E402
from tests import stft_inventory  # noqa: E402
from tests.fir_gpu_harness import ROW_MAX, ROW_REL_L2  # noqa: E402

CSRC = ac.CSRC
LIB = os.path.join(ROOT, "smfft_amd", "libsmfft_stft.so")
SIZES = (256, 512, 1024, 2048, 4096)
LENGTHS = (512, 1024, 2048, 4096, 8192)
FORMS = ("launch", "launch_tuned", "benchmark")
NAMES = ("smfft_stft_fft_size", "smfft_stft_frames") + tuple(f"smfft_{t}_{f}" for t in ("stft", "istft") for f in FORMS)
LDS_BUDGET = 34816             # 4096 / 16 * 17 float2: the transform region of 4096 points; the kernels have no other LDS
NO_DEVICE = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


@pytest.fixture(scope="module")
def stft_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", CSRC, "-j", "4", "../libsmfft_stft.so"])
    return LIB


def _rows(rng, shape):
    return rng.standard_normal(shape).astype(np.float32)


def _spectra(rng, shape):
    """rows of bins with an imaginary part on the two real bins as well: the inverse ignores it"""
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


# ---- 1: the model -------------------------------------------------------------------------------------------
def test_fp64_chain_is_the_direct_sum():
    """n = 512, three Gaussian frames, with a window that has no symmetry and without one: the forward and the inverse chain in fp64
    within 1e-12 of the sums of the definition; the inverse ignores the imaginary parts of bins 0 and M; complex128 / float64 out"""
    n = 512
    rng = np.random.default_rng(250)
    x, X = _rows(rng, (3, n)), _spectra(rng, (3, n // 2 + 1))
    ramp = sm.hann(n) * (1 + np.arange(n) / (2 * n)) + 0.1
    for win in (None, sm.hann(n), ramp):
        got, want = sm.chain(x, win), sm.direct(x, win)
        assert got.shape == (3, n // 2 + 1) and got.dtype == np.complex128
        l2, mx = sm.errors(got, want)
        print(f"forward: fp64 chain relL2 = {l2:.2e}, max = {mx:.2e}")
        assert l2 <= 1e-12 and mx <= 1e-12, (l2, mx)
        assert np.all(got[:, 0].imag == 0) and np.all(got[:, -1].imag == 0)
        assert sm.errors(sm.chain(x, win, power=True), np.abs(want) ** 2)[0] <= 1e-12
        got, want = sm.inverse_chain(X, win), sm.inverse_direct(X, win)
        assert got.shape == (3, n) and got.dtype == np.float64
        l2, mx = sm.errors(got, want)
        print(f"inverse: fp64 chain relL2 = {l2:.2e}, max = {mx:.2e}")
        assert l2 <= 1e-12 and mx <= 1e-12, (l2, mx)
        real_ends = X.copy()
        real_ends[:, [0, -1]] = real_ends[:, [0, -1]].real
        assert np.array_equal(sm.inverse_chain(real_ends, win), got)
    with pytest.raises(ValueError):
        sm.chain(np.zeros(500))
    with pytest.raises(ValueError):
        sm.inverse_chain(np.zeros(252, np.complex64))


def test_fp64_chain_is_numpys_and_torchs():
    """np.fft.rfft / irfft at the five n; torch.stft / torch.istft with center False and True at n = 512 and 2048, an odd hop included:
    torch returns (..., M + 1, frames), ours transposed"""
    import torch
    rng = np.random.default_rng(251)
    for n in LENGTHS:
        x, X, w = _rows(rng, (2, n)), _spectra(rng, (2, n // 2 + 1)), sm.hann(n)
        l2, mx = sm.errors(sm.chain(x, w), np.fft.rfft(x * w))
        assert l2 <= 1e-12 and mx <= 1e-12, (n, l2, mx)
        l2, mx = sm.errors(sm.inverse_chain(X, w), np.fft.irfft(X.astype(np.complex128), n) * w)
        assert l2 <= 1e-12 and mx <= 1e-12, (n, l2, mx)
    for n, hop in ((512, 128), (512, 129), (2048, 512)):
        s = rng.standard_normal((2, 7 * n + 13))
        w = sm.hann(n)
        for center in (False, True):
            want = torch.stft(torch.from_numpy(s), n, hop, window=torch.from_numpy(w), center=center, pad_mode="reflect", onesided=True,
                              return_complex=True).numpy()
            padded = np.pad(s, ((0, 0), (n // 2, n // 2)), mode="reflect") if center else s
            got = sm.chain(sm.frames(padded, n, hop), w)
            assert got.shape == (2, want.shape[2], n // 2 + 1)
            l2, mx = sm.errors(got, want.transpose(0, 2, 1))
            assert l2 <= 1e-12 and mx <= 1e-12, (n, hop, center, l2, mx)
        # the inverse of the centred frames: torch.istft = the overlap-added windowed inverse frames over the summed squared window
        back = torch.istft(torch.from_numpy(want), n, hop, window=torch.from_numpy(w), center=True).numpy()
        mine = sm.overlap_add(sm.inverse_chain(got, w), hop)
        env = sm.overlap_add(np.broadcast_to(w * w, (got.shape[1], n)), hop)
        mine = (mine / np.where(env > 1e-11, env, 1.0))[:, n // 2:mine.shape[1] - n // 2]
        assert mine.shape == back.shape and np.max(np.abs(mine - back)) <= 1e-12, (n, hop)
        assert np.max(np.abs(back - s[:, :back.shape[1]])) <= 1e-12


def test_hann_overlap_add_has_envelope_three_halves_and_reconstructs():
    """the periodic Hann window at hop n / 4: the squared window sums to 1.5 away from the first and the last frame, and the
    overlap-added inverse frames of the forward frames, over 1.5, are the signal there; overlap_add with the window divides by the
    envelope itself and refuses an envelope that reaches zero (Hann starts at 0)"""
    n, hop, F = 512, 128, 12
    w = sm.hann(n)
    assert w[0] == 0 and abs(w[n // 2] - 1) <= 1e-15 and np.max(np.abs(w[1:] - w[:0:-1])) <= 1e-15
    env = sm.overlap_add(np.broadcast_to(w * w, (F, n)), hop)
    assert np.max(np.abs(env[n:-n] - 1.5)) <= 1e-14
    s = np.random.default_rng(252).standard_normal((2, (F - 1) * hop + n))
    fr = sm.frames(s, n, hop)
    assert fr.shape == (2, F, n)
    y = sm.overlap_add(sm.inverse_chain(sm.chain(fr, w), w), hop)
    assert y.shape == s.shape and np.max(np.abs(y[:, n:-n] / 1.5 - s[:, n:-n])) <= 1e-12
    with pytest.raises(ValueError):
        sm.overlap_add(sm.inverse_chain(sm.chain(fr, w), w), hop, w)
    w2 = w + 0.01
    z = sm.overlap_add(sm.inverse_chain(sm.chain(fr, w2), w2), hop, w2, length=s.shape[1] - 5)
    assert z.shape == (2, s.shape[1] - 5) and np.max(np.abs(z - s[:, :-5])) <= 1e-11


def test_fp32_model_is_inside_the_bounds():
    """every stage of the chain rounded to fp32 (the transform itself in fp64, rounded once), n = 512 and 8192: the complex kind and
    the inverse inside the row bounds of the GPU tests, the power inside twice those (d|X|^2 = 2 |X| d|X|)"""
    worst = {}
    for n in (512, 8192):
        rng = np.random.default_rng(253 + n)
        x, X = _rows(rng, (3, n)), _spectra(rng, (3, n // 2 + 1))
        for name, w in (("hann", sm.hann(n, np.float32)), ("no window", None)):
            cases = {"complex": (sm.chain(x, w, np.float32), sm.chain(x, w), 1.0),
                     "power": (sm.chain(x, w, np.float32, power=True), sm.chain(x, w, power=True), 2.0),
                     "inverse": (sm.inverse_chain(X, w, np.float32), sm.inverse_chain(X, w), 1.0)}
            for kind, (got, want, factor) in cases.items():
                assert got.dtype == (np.complex64 if kind == "complex" else np.float32)
                l2, mx = sm.errors(got, want)
                print(f"n={n} {kind}, {name}: fp32 model relL2 = {l2:.2e}, max = {mx:.2e}")
                worst[kind] = [max(a, b) for a, b in zip(worst.get(kind, [0.0, 0.0]), (l2, mx))]
                assert l2 <= factor * ROW_REL_L2 and mx <= factor * ROW_MAX, (n, kind, name, l2, mx)
    for kind, (l2, mx) in worst.items():
        print(f"fp32 model, worst {kind}: relL2 = {l2:.2e}, max |d| / max |want| = {mx:.2e}")
    assert ROW_REL_L2 == 1e-6 and ROW_MAX == 5e-6


def test_source_builds_its_twiddles_from_the_dct_table():
    """W_n^k comes from the fp64-rounded octant of smfft_twiddles_dct.inc through the Rows<M> construction: no table of its own and
    nothing transcendental in the source"""
    # the table lives in the header that the four half-length row libraries share, which includes it exactly once
    source, shared = open(os.path.join(CSRC, "smfft_stft.hip")).read(), open(os.path.join(CSRC, "smfft_rows.hpp")).read()
    assert '#include "smfft/smfft_twiddles_dct.inc"' in shared and shared.count(".inc\"") == 1
    assert '#include "smfft_rows.hpp"' in source and not re.search(r'#include "[^"]*\.inc"', source)
    assert "wn[k] = w32768(k * (16384 / M))" in source
    for text in (source, shared):
        assert not re.search(r"\b(sinf?|cosf?|sincosf?|__sinf|__cosf)\s*\(", re.sub(r"//[^\n]*", "", text))
    for n in LENGTHS:
        assert (n // 2 - 1) * (16384 // (n // 2)) < 16384


# ---- 2: ISA budget and inventory -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """{M: assembly of smfft_stft_<M>.o as the Makefile compiles it}"""
    if not os.path.exists(ac.HIPCC):
        pytest.skip("hipcc not installed")
    # what ships, and the same source with the sample loads marked non-temporal, which tells them from the window's and the twiddles'
    return (ac.addon_isa("smfft_stft", "STFT", SIZES, tmp_path_factory.mktemp("stft_isa")),
            ac.addon_isa("smfft_stft", "STFT", SIZES, tmp_path_factory.mktemp("stft_isa_marked"), extra=["-DSMFFT_STFT_NT_LOAD=1"]))


def test_isa_budget_of_what_ships(isa):
    """per M exactly the three kernels, read from the compiled object's metadata: no scratch, at most 256 VGPRs (two waves per SIMD),
    static LDS of exactly 34,816 B (the transform region of 4096 points: no table in LDS), no transcendentals; the forward kernels
    issue every global load -- plain ones, the shipped policy: samples, window, twiddles -- ahead of the first store, and built with
    the sample loads marked non-temporal they show those as 16 loads of 8 bytes ahead of the first store; the inverse kernel loads
    its 16 bins and bin M non-temporally with 8-byte loads ahead of its first store; the stores are non-temporal, 8 bytes per element
    for the complex kind and the inverse, 4 for the power"""
    total = 0
    shipped, marked = isa
    for m, text in marked.items():
        for name, body in ac.pfb_kernels(text, r"\d+stft_kernel").items():
            rows = [i for i, line in enumerate(body) if re.match(r"global_load_dwordx2\s", line) and re.search(r"\bnt\b", line)]
            nt = [i for i, line in enumerate(body) if line.startswith("global_load") and re.search(r"\bnt\b", line)]
            assert len(rows) == 16 and nt == rows, (name, len(rows), len(nt))
            assert max(rows) < min(i for i, line in enumerate(body) if line.startswith("global_store")), name
    for m, text in shipped.items():
        descs = ac.descriptors(text)
        kernels = {}
        for family, count in (("stft", 2), ("istft", 1)):
            found = ac.pfb_kernels(text, r"\d+%s_kernel" % family)
            assert len(found) == count, (m, family, sorted(found))
            kernels.update({name: (family, body) for name, body in found.items()})
        assert len(descs) == 3 and set(descs) == set(kernels), (m, sorted(descs))
        total += len(descs)
        assert not re.search(r"\bscratch_", text), m
        for name, (family, body) in kernels.items():
            assert re.search(r"%s_kernelILi%dE" % (family, m), name)
            power = family == "stft" and "ELi1EEE" in name
            assert not [line for line in body if re.match(r"v_(sin|cos)_", line)], name
            assert ac.descriptor_field(descs, name, "private_segment_fixed_size") == 0, name
            v, lds = ac.descriptor_field(descs, name, "next_free_vgpr"), ac.descriptor_field(descs, name, "group_segment_fixed_size")
            label = "istft_kernel" if family == "istft" else f"stft_kernel, kind {int(power)}"
            print(f"M={m}: {label}: {v} VGPRs ({ac.occupancy(v)} waves per SIMD), {lds} B of LDS, 0 B of scratch")
            assert lds == LDS_BUDGET and 2 * lds <= ac.LDS_PER_CU, (name, lds)
            assert v <= 256 and ac.occupancy(v) >= 2, (name, v)
            loads = [i for i, line in enumerate(body) if line.startswith("global_load")]
            stores = [i for i, line in enumerate(body) if line.startswith("global_store")]
            rows = [i for i in loads if re.search(r"\bnt\b", body[i])]             # the inverse's bins: non-temporal; the rest: plain
            assert len(rows) == (17 if family == "istft" else 0) and all(re.match(r"global_load_dwordx2\s", body[i]) for i in rows), (name, len(rows))
            # the rest: 16 of the window, 16 of W_n, the engine's own rows, and the forward kernels' 16 of the samples
            assert len(loads) - len(rows) >= (32 if family == "istft" else 48), (name, len(loads))
            rows = rows if family == "istft" else loads
            assert len(stores) == (16 if family == "istft" else 17), (name, len(stores))
            width = r"global_store_dword\s" if power else r"global_store_dwordx2\s"
            assert all(re.match(width, body[i]) and re.search(r"\bnt\b", body[i]) for i in stores), name
            assert min(stores) > max(rows), name
    assert total == 15


def test_library_ships_fifteen_kernels_and_the_inventory_names_them(stft_lib):
    ac.check_inventory(stft_lib, stft_inventory.KERNELS, "smfft_", 15, kinds=("tests", "bounds", "probes"))
    assert len(stft_inventory.KERNELS) == 15
    for family in stft_inventory.FAMILIES:
        assert all(e["call"].startswith(f"smfft_{family}_launch") for k, e in stft_inventory.KERNELS.items() if f"::{family}_kernel<" in k)
    assert "permlane" in stft_inventory.__doc__ and "hostsim" in stft_inventory.__doc__ and "rowconv_real_inventory" in stft_inventory.__doc__


def test_isa_identity_compares_the_library():
    """tools/isa_identity.py compiles the five objects with the Makefile's flags and -I., like the other add-ons' (the tool itself
    needs the history of a git checkout and minutes of compiling: it is run by hand, DESIGN.md section 25 has its verdict)"""
    ac.check_isa_identity_lists("smfft_stft", "STFT", SIZES)
    assert all("-ffp-contract=on" in ac.makefile_flags("STFT", m) for m in SIZES)


# ---- 3: declarations and exports ---------------------------------------------------------------------------------
def test_python_mirror_matches_header(stft_lib):
    from smfft_amd import stft
    header = re.sub(r"[\s*]+", " ", open(os.path.join(ROOT, "include", "smfft_stft.h")).read())
    for phrase in ("X[k] = sum_{j<n} w[j] x[j] exp(-2 pi i jk / n), k = 0 ... M", "torch.stft(..., center=False, onesided=True) transposed",
                   "kind 0 stores X[k] (complex64), kind 1 stores |X[k]|^2 = re re + im im (float32)",
                   "The imaginary parts of X[0] and X[M] are exactly +0", "y[j] = w[j] irfft_n(X)[j]",
                   "The imaginary parts of X[0] and X[M] are ignored", "1/n is a power of two", "NULL means all ones",
                   "X[k] = (Z[k] + P[k]) / 2 - (i/2) W_n^k (Z[k] - P[k])", "Z'[k] = (A + B) + i conj(W_n^k) (A - B)",
                   "4-byte alignment for the signal, the window and the float outputs, 8-byte alignment for complex rows",
                   "every output element is written exactly once", "reads in[c stream_stride + f hop ... + n)",
                   "at element (c frames + f) (M + 1) of d_out", "Frames may overlap each other", "hop may be any value >= 1, odd included",
                   "in[0, (streams-1) stream_stride + (frames-1) hop + n) nor the window",
                   "row r reads M + 1 complex64 at element r (M + 1) and writes n floats at r n", "There is no overlap-add in the kernel",
                   "allocate nothing and do not synchronise", "depend only on that frame, the window, n and the kind",
                   "A NaN or Inf stays in the frames that contain the sample", "a kind outside {0, 1}", "hop < 1 or stream_stride < 1",
                   "grid < 1 (launch_tuned)", "a forbidden overlap", "A zero count launches nothing and returns 0", "Out of scope",
                   "center padding in the kernel", "two-sided output", "n < 512", "not a power of two",
                   "overlap-add inside the inverse kernel", "sums over frames (Welch)", "any element type but float32 / complex64"):
        assert re.sub(r"[\s*]+", " ", phrase) in header, phrase
    decl = ac.declarations("smfft_stft.h")
    assert sorted(decl) == sorted(stft.SIGS) == sorted(NAMES)
    for name, (res, args) in decl.items():
        assert stft.SIGS[name] == ac.signature(res, args), name
    assert stft.SIZES == SIZES and stft.LENGTHS == LENGTHS
    for f in ("stft", "spectrogram", "istft_frames", "overlap_add", "istft", "hann", "launch", "launch_ptr", "istft_ptr", "stft_benchmark",
              "istft_benchmark", "frames", "fft_size"):
        assert callable(getattr(stft, f)), f
    assert "plain torch" in stft.overlap_add.__doc__.lower() and "1e-11" in stft.overlap_add.__doc__


def test_library_exports_exactly_the_eight_symbols(stft_lib):
    ac.check_exports(stft_lib, NAMES)
    assert len(NAMES) == 8


# ---- 4: rejections -------------------------------------------------------------------------------------------------
def test_unsupported_combinations_return_minus_one_without_a_device(stft_lib):
    """-1 (or 0 for a zero count) before any HIP call: run in a process where no GPU is visible, with addresses that are never read.
    Every n next to the five, kind -1 and 2, negative counts, hop 0, stream_stride 0, grid 0, the output starting inside the input
    range, at its last float and on the window; and smfft_stft_frames at L = n - 1, n, n + hop - 1 and n + hop"""
    code = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
ll, d, vp, i = ctypes.c_longlong, ctypes.c_double, ctypes.c_void_p, ctypes.c_int
dp = ctypes.POINTER(d)
S, I = [vp, vp, vp, i, ll, ll, ll, ll, i], [vp, vp, vp, i, ll]
for name, head in (("stft", S), ("istft", I)):
    getattr(lib, f"smfft_{name}_launch").argtypes = head + [vp]
    getattr(lib, f"smfft_{name}_launch_tuned").argtypes = head + [vp, i]
    getattr(lib, f"smfft_{name}_benchmark").argtypes = head + [dp]
lib.smfft_stft_frames.restype, lib.smfft_stft_frames.argtypes = ll, [ll, i, ll]
t = d(0.0)
IN, OUT, WIN = 1 << 30, 1 << 40, 1 << 20
def forms(name, args, grid=3):
    return [getattr(lib, f"smfft_{name}_launch")(*args, None), getattr(lib, f"smfft_{name}_launch_tuned")(*args, None, grid),
            getattr(lib, f"smfft_{name}_benchmark")(*args, ctypes.byref(t))]
def stft(n, streams, frames, hop, stride, kinds=(0, 1), grid=3, din=IN, dout=OUT, win=WIN):
    return [r for kind in kinds for r in forms("stft", (din, dout, win, n, streams, frames, hop, stride, kind), grid)]
def istft(n, batch, grid=3, din=IN, dout=OUT, win=WIN):
    return forms("istft", (din, dout, win, n, batch), grid)
rc, frames = [], []
for n in (256, 500, 16384, 0, -512, 511, 513, 1000, 1023, 1025, 2047, 2049, 4095, 4097, 8191, 8193, 2**31 - 1):
    rc += stft(n, 2, 5, 128, 4096) + stft(n, 0, 0, 128, 4096) + istft(n, 10) + istft(n, 0)
    rc += [lib.smfft_stft_fft_size(n), lib.smfft_stft_frames(1 << 20, n, 128)]
for n in (512, 8192):
    hop = n // 4
    rc += stft(n, 2, 5, hop, 6 * n, kinds=(-1, 2, 7)) + stft(n, 0, 5, hop, 6 * n, kinds=(-1, 2))
    rc += istft(n, -1) + istft(n, -2**40) + istft(n, 2**62)
    rc += stft(n, -1, 5, hop, 6 * n) + stft(n, 2, -1, hop, 6 * n) + stft(n, -1, 0, hop, 6 * n) + stft(n, 0, -1, hop, 6 * n)
    rc += stft(n, 2, 5, 0, 6 * n) + stft(n, 2, 5, -hop, 6 * n) + stft(n, 2, 5, hop, 0) + stft(n, 2, 5, hop, -1) + stft(n, 0, 5, 0, 6 * n) + stft(n, 2, 0, hop, 0)
    rc += stft(n, 2**40, 2**40, hop, 6 * n)
    # stft, 2 streams of 5 frames at hop n / 4, stride 6 n: the input range is 6 n + 4 hop + n = 8 n floats; the output is
    # 10 (n / 2 + 1) complex values or floats
    extent = 6 * n + 4 * hop + n
    for kind, outs in ((0, 20 * (n // 2 + 1)), (1, 10 * (n // 2 + 1))):
        for off in (0, 4, 4 * (extent - 1), -4, -4 * (outs - 1)):
            rc += stft(n, 2, 5, hop, 6 * n, kinds=(kind,), dout=IN + off)
        for off in (0, 4 * (outs - 1), -4 * (n - 1)):
            rc += stft(n, 2, 5, hop, 6 * n, kinds=(kind,), win=OUT + off)
    # istft, 10 rows: n + 2 floats in, n floats out each
    for off in (0, 4, 4 * (10 * (n + 2) - 1), -4, -4 * (10 * n - 1)):
        rc += istft(n, 10, dout=IN + off)
    for off in (0, 4 * (10 * n - 1), -4 * (n - 1)):
        rc += istft(n, 10, win=OUT + off)
    for grid in (0, -1):
        rc += [lib.smfft_stft_launch_tuned(IN, OUT, WIN, n, streams, 5, hop, 6 * n, kind, None, grid) for streams in (2, 0) for kind in (0, 1)]
        rc += [lib.smfft_istft_launch_tuned(IN, OUT, None, n, batch, None, grid) for batch in (10, 0)]
    rc += [lib.smfft_stft_frames(-1, n, hop), lib.smfft_stft_frames(1 << 20, n, 0), lib.smfft_stft_frames(1 << 20, n, -1)]
    frames += [lib.smfft_stft_frames(L, n, hop) for L in (0, n - 1, n, n + hop - 1, n + hop, n + 7 * hop + 1)]
    frames += [lib.smfft_stft_frames(L, n, 1) for L in (n, n + 5, 2**40)]
empty = []
for n in (512, 1024, 2048, 4096, 8192):
    empty += stft(n, 0, 5, n // 4, 6 * n) + stft(n, 2, 0, n // 4, 6 * n) + stft(n, 0, 0, 1, 1, dout=IN, win=None) + istft(n, 0) + istft(n, 0, dout=IN, win=IN)
sizes = [lib.smfft_stft_fft_size(n) for n in (512, 1024, 2048, 4096, 8192)]
want_frames = [0, 0, 1, 1, 2, 8, 1, 6, 2**40 - 512 + 1, 0, 0, 1, 1, 2, 8, 1, 6, 2**40 - 8192 + 1]
print(len(rc), [r for r in rc if r != -1], [e for e in empty if e != 0], t.value, sizes, frames)
good = rc and rc == [-1] * len(rc) and empty and empty == [0] * len(empty) and t.value == 0.0
sys.exit(0 if good and sizes == [256, 512, 1024, 2048, 4096] and frames == want_frames else 1)
"""
    p = subprocess.run([sys.executable, "-c", code, stft_lib], capture_output=True, text=True, timeout=120, env=dict(os.environ, **NO_DEVICE))
    assert p.returncode == 0, p.stdout + p.stderr


def test_python_wrappers_refuse_before_a_device(stft_lib):
    """in a process where no GPU is visible: the pointer forms turn the library's -1 into a RuntimeError, the tensor forms raise
    ValueError or TypeError themselves -- float64, wrong ranks, non-contiguous tensors, windows of another length, tensors on the
    host -- a zero count is served, and overlap_add / hann / frames are what they say"""
    code = ac.REFUSED + r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from smfft_amd import stft
IN, OUT, WIN = 1 << 30, 1 << 40, 1 << 20
for n in (256, 500, 16384, 0):
    refused(RuntimeError, stft.launch_ptr, IN, OUT, WIN, n, 2, 5, 128, 4096)
    refused(RuntimeError, stft.launch_ptr, IN, OUT, WIN, n, 2, 5, 128, 4096, power=True, grid=3)
    refused(RuntimeError, stft.istft_ptr, IN, OUT, None, n, 10)
    assert stft.stft_benchmark(IN, OUT, WIN, n, 2, 5, 128, 4096) == (-1, 0.0) and stft.istft_benchmark(IN, OUT, WIN, n, 10) == (-1, 0.0)
    refused(ValueError, stft.fft_size, n)
    refused(ValueError, stft.frames, 1 << 20, n, 128)
    refused(ValueError, stft.hann, n)
refused(RuntimeError, stft.launch_ptr, IN, OUT, WIN, 512, -1, 5, 128, 4096)
refused(RuntimeError, stft.launch_ptr, IN, OUT, WIN, 512, 2, 5, 0, 4096)
refused(RuntimeError, stft.launch_ptr, IN, OUT, WIN, 512, 2, 5, 128, 0)
refused(RuntimeError, stft.launch_ptr, IN, OUT, WIN, 512, 2, 5, 128, 4096, grid=0)
refused(RuntimeError, stft.launch_ptr, IN, IN + 4, WIN, 512, 2, 5, 128, 4096)
refused(RuntimeError, stft.launch_ptr, IN, OUT, OUT, 512, 2, 5, 128, 4096)
refused(RuntimeError, stft.istft_ptr, IN, IN, None, 512, 10)
refused(RuntimeError, stft.istft_ptr, IN, OUT, None, 512, 10, grid=-1)
refused(ValueError, stft.frames, -1, 512, 128)
refused(ValueError, stft.frames, 4096, 512, 0)
assert [stft.frames(L, 512, 128) for L in (0, 511, 512, 639, 640)] == [0, 0, 1, 1, 2] and stft.fft_size(8192) == 4096
import torch
sig = torch.zeros(2, 4096)
for f in (stft.stft, stft.spectrogram, stft.launch):
    refused(TypeError, f, np.zeros((2, 4096), np.float32), 512, 128)
    refused(TypeError, f, sig.double(), 512, 128)
    refused(ValueError, f, sig, 500, 128)
    refused(ValueError, f, sig, 512, 0)
    refused(ValueError, f, torch.zeros(2, 2, 4096), 512, 128)             # three axes
    refused(ValueError, f, torch.zeros(2, 500), 512, 128)                 # shorter than a frame
    refused(ValueError, f, torch.zeros(2, 8192)[:, ::2], 512, 128)        # not contiguous
    refused(ValueError, f, sig, 512, 128, torch.zeros(256))               # a window of another length
    refused(TypeError, f, sig, 512, 128, torch.zeros(512, dtype=torch.float64))
    refused(TypeError, f, sig, 512, 128, np.zeros(512, np.float32))
    refused(ValueError, f, sig, 512, 128)                                 # a tensor on the host: no CPU fallback
refused(ValueError, stft.stft, sig, 512, 128, None, False, True)          # ... and after the padding of center=True as well
refused(ValueError, stft.stft, torch.zeros(2, 200), 512, 128, center=True)
bins = torch.zeros(2, 5, 257, dtype=torch.complex64)
refused(TypeError, stft.istft_frames, torch.zeros(2, 5, 257))
refused(TypeError, stft.istft_frames, bins.to(torch.complex128))
refused(ValueError, stft.istft_frames, torch.zeros(2, 5, 256, dtype=torch.complex64))
refused(ValueError, stft.istft_frames, torch.zeros(2, 5, 514, dtype=torch.complex64)[:, :, ::2])
refused(ValueError, stft.istft_frames, bins, torch.zeros(256))
refused(ValueError, stft.istft_frames, bins)
refused(ValueError, stft.istft, bins, 128, torch.ones(512))
w = stft.hann(512)
assert w.dtype == torch.float32 and w.shape == (512,)
assert np.array_equal(w.numpy(), (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(512) / 512)).astype(np.float32))
assert torch.allclose(w, torch.hann_window(512, periodic=True), atol=2e-7, rtol=0)
y = stft.overlap_add(torch.arange(12.0).reshape(3, 4), 2)
assert y.tolist() == [0.0, 1.0, 2.0 + 4.0, 3.0 + 5.0, 6.0 + 8.0, 7.0 + 9.0, 10.0, 11.0]
assert stft.overlap_add(torch.arange(12.0).reshape(3, 4), 2, length=5).tolist() == [0.0, 1.0, 6.0, 8.0, 14.0]
assert stft.overlap_add(torch.arange(12.0).reshape(3, 4), 2, length=10).tolist() == [0.0, 1.0, 6.0, 8.0, 14.0, 16.0, 10.0, 11.0, 0.0, 0.0]
assert stft.overlap_add(torch.arange(12.0).reshape(3, 4), 2, center=True).tolist() == [6.0, 8.0, 14.0, 16.0]
two = torch.full((4,), 2.0)
assert stft.overlap_add(torch.ones(2, 3, 4), 2, two).tolist() == [[0.25, 0.25, 0.25, 0.25, 0.25, 0.25, 0.25, 0.25]] * 2
refused(ValueError, stft.overlap_add, torch.ones(3, 4), 2, torch.tensor([0.0, 1.0, 1.0, 1.0]))      # the envelope reaches zero
refused(ValueError, stft.overlap_add, torch.ones(3, 4), 0)
stft.launch_ptr(IN, OUT, None, 512, 0, 5, 128, 4096)                      # an empty batch: nothing is launched
stft.istft_ptr(IN, OUT, None, 8192, 0)
assert stft.stft_benchmark(IN, OUT, None, 512, 2, 0, 128, 4096, power=True) == (0, 0.0)
print("ok")
"""
    p = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300, env=dict(os.environ, **NO_DEVICE))
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout + p.stderr


def test_import_does_not_load_the_library():
    ac.check_import_does_not_load("stft", "smfft_stft")

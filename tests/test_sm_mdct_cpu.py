"""CPU checks of the DCT-IV / MDCT library (smfft_amd/csrc/smfft_mdct.hip, libsmfft_mdct.so): the model's chain (tools/mdct_model.py)
in fp64 is the fp64 sum of the definition and scipy's type 4 transforms, the MDCT / IMDCT are their sums and cancel their aliasing, and
in fp32 the chain stays inside the GPU tests' bounds; the fold and the unfold cover every sample once; the generated twiddle table is
the committed one and its symmetric extension gives fp64 values rounded once; the gfx950 code of the fifteen kernels keeps its budget;
and the C ABI declares, exports and validates the ten entry points without a device.  No GPU code is run (hipcc cross-compiles gfx950)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_twiddles_mdct  # noqa: E402
import mdct_model as mm  # noqa: E402

from tests import addon_checks as ac  # noqa: E402
from tests import mdct_inventory  # noqa: E402
from tests.fir_gpu_harness import ROW_MAX, ROW_REL_L2  # noqa: E402

CSRC = ac.CSRC
LIB = os.path.join(ROOT, "smfft_amd", "libsmfft_mdct.so")
SIZES = (256, 512, 1024, 2048, 4096)
LENGTHS = (512, 1024, 2048, 4096, 8192)
FORMS = ("launch", "launch_tuned", "benchmark")
NAMES = ("smfft_mdct_fft_size",) + tuple(f"smfft_{t}_{f}" for t in ("dct4", "mdct", "imdct") for f in FORMS)
LDS_BUDGET = 34816             # 4096 / 16 * 17 float2: the transform region of 4096 points; the kernels have no other LDS
NO_DEVICE = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


@pytest.fixture(scope="module")
def mdct_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", CSRC, "-j", "4", "../libsmfft_mdct.so"])
    return LIB


def _rows(rng, shape):
    return rng.standard_normal(shape).astype(np.float32)


# ---- 1: the model -------------------------------------------------------------------------------------------
def test_fp64_chain_is_the_direct_sums_and_the_identities_hold():
    """n = 512, three Gaussian rows, and n = 8192, one row: the chain in fp64 within 1e-12 of the cosine and sine sums of the
    definition; DST-IV(x)[k] = (-1)^k DCT-IV(reverse x)[k]; each transform is its own inverse up to 2n; float64 out"""
    n = 512
    x = _rows(np.random.default_rng(240), (3, n))
    s = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    for sine in (False, True):
        want, got = mm.direct(x, sine), mm.chain(x, sine)
        assert got.shape == x.shape and got.dtype == np.float64
        l2, mx = mm.errors(got, want)
        print(f"sine {sine}: fp64 chain relL2 = {l2:.2e}, max = {mx:.2e}")
        assert l2 <= 1e-12 and mx <= 1e-12, (sine, l2, mx)
        assert mm.errors(mm.direct(mm.direct(x, sine), sine) / (2 * n), x)[0] <= 1e-12
        assert mm.errors(mm.chain(mm.chain(x, sine), sine) / (2 * n), x)[0] <= 1e-12
    assert mm.errors(mm.direct(x, True), s * mm.direct(x[:, ::-1], False))[0] <= 1e-13
    # n = 8192 against the direct sums as well (one row: the 8192 x 8192 matrix of the definition), whether scipy is there or not
    x = _rows(np.random.default_rng(2408), (1, 8192))
    for sine in (False, True):
        l2, mx = mm.errors(mm.chain(x, sine), mm.direct(x, sine))
        print(f"n=8192 sine {sine}: fp64 chain relL2 = {l2:.2e}, max = {mx:.2e}")
        assert l2 <= 1e-12 and mx <= 1e-12, (8192, sine, l2, mx)
    with pytest.raises(ValueError):
        mm.chain(np.zeros(500))
    with pytest.raises(ValueError):
        mm.mdct_chain(np.zeros(512))


def test_fp64_chain_is_scipys():
    """scipy.fft.dct / dst with norm=None, type 4, at n = 512 and 8192"""
    sf = pytest.importorskip("scipy.fft")
    for n in (512, 8192):
        x = _rows(np.random.default_rng(241 + n), (2, n))
        for sine in (False, True):
            want = (sf.dst if sine else sf.dct)(x.astype(np.float64), type=4, axis=-1)
            l2, mx = mm.errors(mm.chain(x, sine), want)
            assert l2 <= 1e-12 and mx <= 1e-12, (n, sine, l2, mx)


def test_mdct_and_imdct_are_their_sums_and_cancel_their_aliasing():
    """N = 512: the chains within 1e-12 of the sums of the definition, with a window and without; and with the sine window,
    w[j]^2 + w[j+N]^2 = 1, overlap-adding the IMDCT of the MDCT frames at hop N gives (N/2) x away from the two ends"""
    N = 512
    rng = np.random.default_rng(242)
    x, X = _rows(rng, (3, 2 * N)), _rows(rng, (3, N))
    w = mm.sine_window(N)
    assert np.max(np.abs(w[:N] ** 2 + w[N:] ** 2 - 1)) <= 1e-15
    ramp = w * (1 + np.arange(2 * N) / (4 * N))              # a window with no symmetry of its own
    for win in (None, w, ramp):
        for got, want in ((mm.mdct_chain(x, win), mm.mdct_direct(x, win)), (mm.imdct_chain(X, win), mm.imdct_direct(X, win))):
            assert got.dtype == np.float64
            l2, mx = mm.errors(got, want)
            assert l2 <= 1e-12 and mx <= 1e-12, (l2, mx)
    s = rng.standard_normal((2, 6 * N))
    fr = mm.frames(s, N)
    assert fr.shape == (2, 5, 2 * N)
    y = mm.overlap_add(mm.imdct_chain(mm.mdct_chain(fr, w), w)) / (N / 2)
    assert y.shape == s.shape and np.max(np.abs(y[:, N:-N] - s[:, N:-N])) <= 1e-12
    assert np.max(np.abs(y[:, :N] - s[:, :N])) > 1e-3        # (the ends keep their aliasing)


def test_fp32_model_is_inside_the_bounds():
    """every stage of the chain rounded to fp32 (the transform itself in fp64, rounded once), n = 512 and 8192, the four transforms:
    the row bounds of the GPU tests hold"""
    worst = [0.0, 0.0]
    for n in (512, 8192):
        rng = np.random.default_rng(243 + n)
        x, x2 = _rows(rng, (3, n)), _rows(rng, (3, 2 * n))
        w = mm.sine_window(n, np.float32)
        cases = {"dct4": (mm.chain(x, False, np.float32), mm.chain(x, False)), "dst4": (mm.chain(x, True, np.float32), mm.chain(x, True)),
                 "mdct": (mm.mdct_chain(x2, w, np.float32), mm.mdct_chain(x2, w)), "mdct, no window": (mm.mdct_chain(x2, None, np.float32), mm.mdct_chain(x2)),
                 "imdct": (mm.imdct_chain(x, w, np.float32), mm.imdct_chain(x, w))}
        for name, (got, want) in cases.items():
            assert got.dtype == np.float32
            l2, mx = mm.errors(got, want)
            print(f"n={n} {name}: fp32 model relL2 = {l2:.2e}, max = {mx:.2e}")
            worst = [max(worst[0], l2), max(worst[1], mx)]
            assert l2 <= ROW_REL_L2 and mx <= ROW_MAX, (n, name, l2, mx)
    print(f"fp32 model, worst: relL2 = {worst[0]:.2e}, max |d| / max |want| = {worst[1]:.2e}")
    assert ROW_REL_L2 == 1e-6 and ROW_MAX == 5e-6


def test_fold_and_unfold_cover_every_sample_once():
    """the fold reads each of the 2N samples of a frame exactly once over its two index rows, with the signs of u = [-c_r - d, a - b_r];
    the unfold writes 2N outputs, reads every D exactly twice, and is the transpose of the fold: <fold(v), D> = <v, unfold(D)>"""
    for N in LENGTHS:
        h = N // 2
        i0, s0, i1, s1 = mm.fold_index(N)
        assert np.array_equal(np.sort(np.concatenate([i0, i1])), np.arange(2 * N))
        v = np.arange(2 * N, dtype=np.float64) + 1
        a, b, c, d = v[:h], v[h:N], v[N:N + h], v[N + h:]
        assert np.array_equal(s0 * v[i0] + s1 * v[i1], np.concatenate([-c[::-1] - d, a - b[::-1]]))
        i, s = mm.unfold_index(N)
        assert i.shape == (2 * N,) and np.array_equal(np.bincount(i, minlength=N), np.full(N, 2))
        D = np.arange(N, dtype=np.float64) + 1
        assert np.array_equal(s * D[i], np.concatenate([D[h:], -D[::-1], -D[:h]]))
        assert np.dot(s0 * v[i0] + s1 * v[i1], D) == np.dot(v, s * D[i])


def test_twiddle_table_is_the_generated_one():
    """the committed table is the generator's text and no larger than the octant of W_32768; the extension that the kernels'
    compile-time rows apply gives, over the whole quarter circle of W_65536, values within half an ulp of one of fp64's (2^-25, with
    one per cent for the second rounding of the mirrored entries); the source applies those symmetries and nothing transcendental"""
    path = os.path.join(ROOT, "include", "smfft", "smfft_twiddles_mdct.inc")
    assert os.path.abspath(gen_twiddles_mdct.PATH) == os.path.abspath(path)
    assert open(path).read() == gen_twiddles_mdct.table_text()
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(ROOT, "include", "smfft", "smfft_twiddles_dct.inc"))
    c, s = gen_twiddles_mdct.quarter_table()
    ang = 2 * np.pi * np.arange(16384) / 65536
    assert np.max(np.abs(c.astype(np.float64) - np.cos(ang))) <= 1.01 * 2.0 ** -25
    assert np.max(np.abs(s.astype(np.float64) - np.sin(ang))) <= 1.01 * 2.0 ** -25
    assert c[0] == 1 and s[0] == 0 and c[8192] == s[8192]
    # what the rows index: (4p+1) 8192 / n of W_65536 and k 16384 / n of W_32768 stay inside the quarter and the half circle
    for n in LENGTHS:
        assert (4 * (n // 2 - 1) + 1) * (8192 // n) < 16384 and (n // 2 - 1) * (16384 // n) < 16384
    # W_65536 is this library's own; W_32768 comes from the header that the four half-length row libraries share
    source, shared = open(os.path.join(CSRC, "smfft_mdct.hip")).read(), open(os.path.join(CSRC, "smfft_rows.hpp")).read()
    assert '#include "smfft/smfft_twiddles_mdct.inc"' in source and '#include "smfft_rows.hpp"' in source
    assert '#include "smfft/smfft_twiddles_dct.inc"' in shared
    assert "TwiddleValue{b.y, b.x}" in source and "odd_octant_65536[(16384 - m - 1) / 2]" in source
    for text in (source, shared):
        assert not re.search(r"\b(sinf?|cosf?|sincosf?|__sinf|__cosf)\s*\(", re.sub(r"//[^\n]*", "", text))


# ---- 2: ISA budget and inventory -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """{M: assembly of smfft_mdct_<M>.o as the Makefile compiles it}"""
    if not os.path.exists(ac.HIPCC):
        pytest.skip("hipcc not installed")
    return ac.addon_isa("smfft_mdct", "MDCT", SIZES, tmp_path_factory.mktemp("mdct_isa"))


def test_isa_budget_of_what_ships(isa):
    """per M exactly the three kernels, read from the compiled object's metadata: no scratch, at most 256 VGPRs (two waves per SIMD),
    static LDS of exactly 34,816 B (the transform region of 4096 points: no table in LDS), no transcendentals; the row accesses are
    16 bytes wide -- 8 loads and 8 stores (dct4), 16 sample loads, 16 window loads and 8 stores (mdct), 8 loads, 16 window loads and
    16 stores (imdct) per thread -- and every row load precedes the first store"""
    total = 0
    counts = {"dct4": (8, 8), "mdct": (32, 8), "imdct": (24, 16)}
    for m, text in isa.items():
        descs = ac.descriptors(text)
        kernels = {}
        for family in mdct_inventory.FAMILIES:
            found = ac.pfb_kernels(text, r"\d+%s_kernel" % family)
            assert len(found) == 1, (m, family, sorted(found))
            kernels.update({name: (family, body) for name, body in found.items()})
        assert len(descs) == 3 and set(descs) == set(kernels), (m, sorted(descs))
        total += len(descs)
        assert not re.search(r"\bscratch_", text), m
        for name, (family, body) in kernels.items():
            assert re.search(r"%s_kernelILi%dE" % (family, m), name)
            assert not [line for line in body if re.match(r"v_(sin|cos)_", line)], name
            assert ac.descriptor_field(descs, name, "private_segment_fixed_size") == 0, name
            v, lds = ac.descriptor_field(descs, name, "next_free_vgpr"), ac.descriptor_field(descs, name, "group_segment_fixed_size")
            print(f"M={m}: {family}_kernel {v} VGPRs ({ac.occupancy(v)} waves per SIMD), {lds} B of LDS, 0 B of scratch")
            assert lds == LDS_BUDGET and 2 * lds <= ac.LDS_PER_CU, (name, lds)
            assert v <= 256 and ac.occupancy(v) >= 2, (name, v)
            # the row (and window) accesses are the 16-byte ones; the 8-byte loads are twiddles
            loads = [i for i, line in enumerate(body) if re.match(r"global_load_dwordx4\s", line)]
            stores = [i for i, line in enumerate(body) if line.startswith("global_store")]
            assert (len(loads), len(stores)) == counts[family], (name, len(loads), len(stores))
            assert all(re.match(r"global_store_dwordx4\s", body[i]) for i in stores), name
            assert not [line for line in body if re.match(r"global_load_dword\s", line)], name
            rows = [i for i in loads if re.search(r"\bnt\b", body[i])]             # the samples: non-temporal; the window: plain
            assert len(rows) == {"dct4": 8, "mdct": 16, "imdct": 8}[family], (name, len(rows))
            assert min(stores) > max(rows), name
    assert total == 15


def test_library_ships_fifteen_kernels_and_the_inventory_names_them(mdct_lib):
    ac.check_inventory(mdct_lib, mdct_inventory.KERNELS, "smfft_", 15, kinds=("tests", "bounds", "probes"))
    assert len(mdct_inventory.KERNELS) == 15
    for family in mdct_inventory.FAMILIES:
        assert all(e["call"].startswith(f"smfft_{family}_launch") for k, e in mdct_inventory.KERNELS.items() if f"::{family}_kernel<" in k)
    assert "permlane" in mdct_inventory.__doc__ and "hostsim" in mdct_inventory.__doc__


def test_isa_identity_compares_the_library():
    """tools/isa_identity.py compiles the five objects with the Makefile's flags and -I., like the other add-ons' (the tool itself
    needs the history of a git checkout and minutes of compiling: it is run by hand, DESIGN.md section 24 has its verdict)"""
    ac.check_isa_identity_lists("smfft_mdct", "MDCT", SIZES)
    assert all("-ffp-contract=on" in ac.makefile_flags("MDCT", m) for m in SIZES)


# ---- 3: declarations and exports ---------------------------------------------------------------------------------
def test_python_mirror_matches_header(mdct_lib):
    from smfft_amd import mdct
    header = re.sub(r"[\s*]+", " ", open(os.path.join(ROOT, "include", "smfft_mdct.h")).read())
    for phrase in ("the type IV transforms follow the convention of scipy.fft with norm=None", "X[k] = 2 sum_j x[j] cos(pi (2k+1)(2j+1) / (4n))",
                   "X[k] = 2 sum_j x[j] sin(pi (2k+1)(2j+1) / (4n))", "(-1)^k DCT-IV(reverse x)[k]", "DCT-IV(DCT-IV(x)) = 2n x",
                   "X[k] = sum_{j<2N} w[j] x[j] cos(pi/N (j + 1/2 + N/2)(k + 1/2))", "y[j] = w[j] sum_{k<N} X[k] cos(pi/N (j + 1/2 + N/2)(k + 1/2))",
                   "w[j]^2 + w[j+N]^2 = 1", "gives (N/2) x", "NULL means all ones", "In place, d_out == d_in, is allowed",
                   "Ranges that overlap without being equal are refused", "4-byte alignment", "every output element is written exactly once",
                   "reads in[c stream_stride + f hop ... + 2N)", "writes out[(c frames + f) N ... + N)", "Frames may overlap each other",
                   "depend only on that row or frame (and the window), n and the transform", "A NaN or Inf in a row or frame stays in it",
                   "A zero count launches nothing and returns 0", "hop < 1 or stream_stride < 1", "Out of scope", "type I",
                   "orthonormal scaling", "overlap-add inside the IMDCT kernel", "windows other than caller-supplied tables"):
        assert phrase in header, phrase
    decl = ac.declarations("smfft_mdct.h")
    assert sorted(decl) == sorted(mdct.SIGS) == sorted(NAMES)
    for name, (res, args) in decl.items():
        assert mdct.SIGS[name] == ac.signature(res, args), name
    assert mdct.SIZES == SIZES and mdct.LENGTHS == LENGTHS
    for f in ("dct4", "dst4", "mdct", "mdct_frames", "imdct", "overlap_add", "sine_window", "launch_ptr", "dct4_ptr", "mdct_ptr", "imdct_ptr"):
        assert callable(getattr(mdct, f)), f
    assert "plain torch" in mdct.overlap_add.__doc__.lower()


def test_library_exports_exactly_the_ten_symbols(mdct_lib):
    ac.check_exports(mdct_lib, NAMES)
    assert len(NAMES) == 10


# ---- 4: rejections -------------------------------------------------------------------------------------------------
def test_unsupported_combinations_return_minus_one_without_a_device(mdct_lib):
    """-1 (or 0 for a zero count) before any HIP call: run in a process where no GPU is visible, with addresses that are never read.
    Every length next to the five, negative counts, hop < 1, stream_stride < 1, grid < 1, and every forbidden overlap: dct4's ranges
    overlapping without being equal, the MDCT's and the IMDCT's output inside the input range or on the window"""
    code = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
ll, d, vp, i = ctypes.c_longlong, ctypes.c_double, ctypes.c_void_p, ctypes.c_int
dp = ctypes.POINTER(d)
D, M, I = [vp, vp, i, ll, i], [vp, vp, vp, i, ll, ll, ll, ll], [vp, vp, vp, i, ll]
for name, head in (("dct4", D), ("mdct", M), ("imdct", I)):
    getattr(lib, f"smfft_{name}_launch").argtypes = head + [vp]
    getattr(lib, f"smfft_{name}_launch_tuned").argtypes = head + [vp, i]
    getattr(lib, f"smfft_{name}_benchmark").argtypes = head + [dp]
t = d(0.0)
IN, OUT, WIN = 1 << 30, 1 << 40, 1 << 20
def forms(name, args, grid=3):
    return [getattr(lib, f"smfft_{name}_launch")(*args, None), getattr(lib, f"smfft_{name}_launch_tuned")(*args, None, grid),
            getattr(lib, f"smfft_{name}_benchmark")(*args, ctypes.byref(t))]
def dct4(n, batch, grid=3, din=IN, dout=OUT):
    return [r for s in (0, 1, 7) for r in forms("dct4", (din, dout, n, batch, s), grid)]
def mdct(N, streams, frames, hop, stride, grid=3, din=IN, dout=OUT, win=WIN):
    return forms("mdct", (din, dout, win, N, streams, frames, hop, stride), grid)
def imdct(N, batch, grid=3, din=IN, dout=OUT, win=WIN):
    return forms("imdct", (din, dout, win, N, batch), grid)
rc = []
for n in (256, 500, 16384, 0, -512, 513, 1000, 8191, 2**31 - 1):
    rc += dct4(n, 10) + dct4(n, 0) + dct4(n, 10, dout=IN) + mdct(n, 2, 5, 512, 4096) + mdct(n, 0, 0, 512, 4096) + imdct(n, 10) + imdct(n, 0)
    rc += [lib.smfft_mdct_fft_size(n)]
for n in (512, 8192):
    rc += dct4(n, -1) + dct4(n, -2**40) + imdct(n, -1) + imdct(n, -2**40)
    rc += mdct(n, -1, 5, n, 6 * n) + mdct(n, 2, -1, n, 6 * n) + mdct(n, -1, 0, n, 6 * n) + mdct(n, 0, -1, n, 6 * n)
    rc += mdct(n, 2, 5, 0, 6 * n) + mdct(n, 2, 5, -n, 6 * n) + mdct(n, 2, 5, n, 0) + mdct(n, 2, 5, n, -1) + mdct(n, 0, 5, 0, 6 * n) + mdct(n, 2, 0, n, 0)
    rc += mdct(n, 2**40, 2**40, n, 6 * n) + dct4(n, 2**62) + imdct(n, 2**62)
    # dct4: overlapping, unequal: the output starts inside the input, ends inside it, or one element off
    for off in (4, 4 * n, 4 * (10 * n - 1), -4, -4 * (10 * n - 1)):
        rc += dct4(n, 10, dout=IN + off)
    # mdct, 2 streams of 5 frames at hop n, stride 6 n: the input range is 12 n floats, the output 10 n floats
    for off in (0, 4, 4 * (12 * n - 1), -4, -4 * (10 * n - 1)):
        rc += mdct(n, 2, 5, n, 6 * n, dout=IN + off)
    for off in (0, 4 * (10 * n - 1), -4 * (2 * n - 1)):
        rc += mdct(n, 2, 5, n, 6 * n, win=OUT + off)
    # imdct, 10 rows: n floats in, 2 n floats out each
    for off in (0, 4, 4 * (10 * n - 1), -4, -4 * (20 * n - 1)):
        rc += imdct(n, 10, dout=IN + off)
    for off in (0, 4 * (20 * n - 1), -4 * (2 * n - 1)):
        rc += imdct(n, 10, win=OUT + off)
    for grid in (0, -1):
        rc += [lib.smfft_dct4_launch_tuned(IN, OUT, n, batch, 0, None, grid) for batch in (10, 0)]
        rc += [lib.smfft_dct4_launch_tuned(IN, IN, n, batch, 0, None, grid) for batch in (10, 0)]
        rc += [lib.smfft_mdct_launch_tuned(IN, OUT, WIN, n, streams, 5, n, 6 * n, None, grid) for streams in (2, 0)]
        rc += [lib.smfft_imdct_launch_tuned(IN, OUT, None, n, batch, None, grid) for batch in (10, 0)]
empty = []
for n in (512, 1024, 2048, 4096, 8192):
    empty += dct4(n, 0) + dct4(n, 0, dout=IN) + dct4(n, 0, dout=IN + 4) + dct4(n, 0, din=None, dout=None)
    empty += mdct(n, 0, 5, n, 6 * n) + mdct(n, 2, 0, n, 6 * n) + mdct(n, 0, 0, 1, 1, dout=IN, win=None) + imdct(n, 0) + imdct(n, 0, dout=IN, win=IN)
sizes = [lib.smfft_mdct_fft_size(n) for n in (512, 1024, 2048, 4096, 8192)]
print(len(rc), [r for r in rc if r != -1], [e for e in empty if e != 0], t.value, sizes)
sys.exit(0 if rc and rc == [-1] * len(rc) and empty and empty == [0] * len(empty) and t.value == 0.0 and sizes == [256, 512, 1024, 2048, 4096] else 1)
"""
    p = subprocess.run([sys.executable, "-c", code, mdct_lib], capture_output=True, text=True, timeout=120, env=dict(os.environ, **NO_DEVICE))
    assert p.returncode == 0, p.stdout + p.stderr


def test_python_wrappers_refuse_before_a_device(mdct_lib):
    """in a process where no GPU is visible: the pointer forms turn the library's -1 into a RuntimeError, the tensor and array forms
    raise ValueError or TypeError themselves, and a zero count is served"""
    code = ac.REFUSED + r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from smfft_amd import mdct
IN, OUT, WIN = 1 << 30, 1 << 40, 1 << 20
for n in (256, 500, 16384, 0):
    refused(RuntimeError, mdct.launch_ptr, IN, OUT, n, 10)
    refused(RuntimeError, mdct.dct4_ptr, IN, OUT, n, 10, grid=3)
    refused(RuntimeError, mdct.mdct_ptr, IN, OUT, WIN, n, 2, 5, 512, 4096)
    refused(RuntimeError, mdct.imdct_ptr, IN, OUT, None, n, 10)
    assert mdct.dct4_benchmark(IN, OUT, n, 10) == (-1, 0.0) and mdct.imdct_benchmark(IN, OUT, WIN, n, 10) == (-1, 0.0)
    assert mdct.mdct_benchmark(IN, OUT, WIN, n, 2, 5, 512, 4096) == (-1, 0.0)
    refused(ValueError, mdct.fft_size, n)
    refused(ValueError, mdct.dct4, np.zeros((2, n), np.float32))
    refused(ValueError, mdct.dst4, np.zeros((2, n), np.float32))
refused(RuntimeError, mdct.launch_ptr, IN, OUT, 512, -1)
refused(RuntimeError, mdct.launch_ptr, IN, IN + 4, 512, 10)
refused(RuntimeError, mdct.dct4_ptr, IN, OUT, 512, 10, grid=0)
refused(RuntimeError, mdct.mdct_ptr, IN, OUT, WIN, 512, 2, 5, 0, 4096)
refused(RuntimeError, mdct.mdct_ptr, IN, OUT, WIN, 512, 2, 5, 512, 0)
refused(RuntimeError, mdct.mdct_ptr, IN, IN + 4, WIN, 512, 2, 5, 512, 4096)
refused(RuntimeError, mdct.mdct_ptr, IN, OUT, OUT, 512, 2, 5, 512, 4096)
refused(RuntimeError, mdct.imdct_ptr, IN, IN, None, 512, 10)
refused(RuntimeError, mdct.imdct_ptr, IN, OUT, None, 512, 10, grid=-1)
refused(TypeError, mdct.dct4, np.zeros((2, 512), np.complex64))
refused(ValueError, mdct.dct4, np.float32(1))
refused(TypeError, mdct.launch, np.zeros((2, 512), np.float32))
import torch
refused(ValueError, mdct.launch, torch.zeros(2, 512))                     # a tensor on the host: no CPU fallback
refused(ValueError, mdct.launch, torch.zeros(2, 500))
refused(TypeError, mdct.launch, torch.zeros(2, 512, dtype=torch.float64))
refused(ValueError, mdct.launch, torch.zeros(2, 1024)[:, ::2])
refused(ValueError, mdct.mdct, torch.zeros(2, 1024))
refused(ValueError, mdct.mdct, torch.zeros(2, 1000))
refused(ValueError, mdct.mdct, torch.zeros(2, 1023))
refused(ValueError, mdct.mdct, torch.zeros(2, 1024), torch.zeros(512))
refused(TypeError, mdct.mdct, torch.zeros(2, 1024), np.zeros(1024, np.float32))
refused(ValueError, mdct.imdct, torch.zeros(2, 512))
refused(ValueError, mdct.imdct, torch.zeros(2, 500))
refused(ValueError, mdct.mdct_frames, torch.zeros(2, 4096), None, 512)
refused(ValueError, mdct.mdct_frames, torch.zeros(2, 4000), None, 512)
refused(ValueError, mdct.mdct_frames, torch.zeros(2, 512), None, 512)
refused(ValueError, mdct.mdct_frames, torch.zeros(4096), None, 512)
refused(ValueError, mdct.mdct_frames, torch.zeros(2, 4096), None, 500)
refused(ValueError, mdct.sine_window, 500)
w = mdct.sine_window(512)
assert w.dtype == torch.float32 and w.shape == (1024,)
want = np.sin(np.pi * (np.arange(1024) + 0.5) / 1024).astype(np.float32)
assert np.array_equal(w.numpy(), want)
y = mdct.overlap_add(torch.arange(12.0).reshape(3, 4))
assert y.tolist() == [0.0, 1.0, 2.0 + 4.0, 3.0 + 5.0, 6.0 + 8.0, 7.0 + 9.0, 10.0, 11.0]
mdct.launch_ptr(IN, IN, 8192, 0, True)                                    # an empty batch, in place: nothing is launched
mdct.mdct_ptr(IN, OUT, None, 512, 0, 5, 512, 4096)
mdct.imdct_ptr(IN, OUT, None, 512, 0)
assert mdct.dct4_benchmark(IN, OUT, 512, 0) == (0, 0.0) and mdct.fft_size(8192) == 4096
print("ok")
"""
    p = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300, env=dict(os.environ, **NO_DEVICE))
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout + p.stderr


def test_import_does_not_load_the_library():
    ac.check_import_does_not_load("mdct", "smfft_mdct")

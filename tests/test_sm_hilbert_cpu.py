"""CPU checks of the Hilbert library (smfft_amd/csrc/smfft_hilbert.hip, libsmfft_hilbert.so): the model's chain (tools/hilbert_model.py)
in fp64 is the definition through the full-length DFT and scipy.signal.hilbert for the three kinds, and in fp32 stays inside the GPU
tests' bounds; the gfx950 code of the fifteen kernels keeps its budget; and the C ABI declares, exports and validates the four entry
points without a device.  No GPU code is run (hipcc cross-compiles gfx950)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import hilbert_model as hm  # noqa: E402

from tests import addon_checks as ac  # noqa: E402
from tests import hilbert_inventory  # noqa: E402
from tests.fir_gpu_harness import ROW_MAX, ROW_REL_L2  # noqa: E402

CSRC = ac.CSRC
LIB = os.path.join(ROOT, "smfft_amd", "libsmfft_hilbert.so")
SIZES = (256, 512, 1024, 2048, 4096)
LENGTHS = (512, 1024, 2048, 4096, 8192)
KINDS = (0, 1, 2)
NAMES = ("smfft_hilbert_fft_size", "smfft_hilbert_launch", "smfft_hilbert_launch_tuned", "smfft_hilbert_benchmark")
LDS_BUDGET = 34816             # 4096 / 16 * 17 float2: the transform region of 4096 points; the kernels have no other LDS
NO_DEVICE = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


@pytest.fixture(scope="module")
def hilbert_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", CSRC, "-j", "4", "../libsmfft_hilbert.so"])
    return LIB


def _rows(rng, shape):
    return rng.standard_normal(shape).astype(np.float32)


# ---- 1: the model -------------------------------------------------------------------------------------------
def test_fp64_chain_is_the_definition():
    """n = 512 and 8192, three Gaussian rows: the chain in fp64 within 1e-12 (relative to the input row, both measures) of the definition
    through the full-length DFT for the three kinds; cos(2 pi 5 j / n) gives sin(2 pi 5 j / n); a row of DC plus Nyquist gives exactly 0,
    in fp64 and in the fp32 model; the analytic kind is complex with the input as its real part, the others are real"""
    for n in (512, 8192):
        x = _rows(np.random.default_rng(230 + n), (3, n))
        for kind in KINDS:
            want, got = hm.direct(x, kind), hm.chain(x, kind)
            assert got.shape == x.shape and got.dtype == (np.complex128 if kind == 1 else np.float64)
            l2, mx = hm.errors(got, want, x)
            print(f"n={n} kind {kind}: fp64 chain relL2 = {l2:.2e}, max = {mx:.2e}")
            assert l2 <= 1e-12 and mx <= 1e-12, (n, kind, l2, mx)
        assert np.array_equal(hm.chain(x, 1).real, x.astype(np.float64))
        assert np.array_equal(hm.chain(x, 1, np.float32).real, x)
        j = np.arange(n)
        tone = np.cos(2 * np.pi * 5 * j / n)[None]
        assert np.abs(hm.chain(tone) - np.sin(2 * np.pi * 5 * j / n)).max() <= 1e-12
        assert np.abs(hm.chain(tone, 2) - 1.0).max() <= 1e-12                     # the envelope of a tone is its amplitude
        flat = (3.0 + 2.0 * (-1.0) ** j)[None]
        assert not hm.chain(flat).any() and not hm.chain(flat, 0, np.float32).any()
        assert np.array_equal(hm.chain(flat, 2), np.abs(flat))
    with pytest.raises(ValueError):
        hm.chain(np.zeros(500))
    with pytest.raises(ValueError):
        hm.chain(np.zeros(512), 3)


def test_fp64_chain_is_scipys():
    """scipy.signal.hilbert at n = 512 and 8192: its imaginary part, itself and its modulus"""
    ss = pytest.importorskip("scipy.signal")
    for n in (512, 8192):
        x = _rows(np.random.default_rng(231 + n), (2, n))
        a = ss.hilbert(x.astype(np.float64), axis=-1)
        for kind, want in ((0, a.imag), (1, a), (2, np.abs(a))):
            l2, mx = hm.errors(hm.chain(x, kind), want, x)
            assert l2 <= 1e-12 and mx <= 1e-12, (n, kind, l2, mx)


def test_fp32_model_is_inside_the_bounds():
    """every stage of the chain rounded to fp32 (the transforms themselves in fp64, rounded once), n = 512 and 8192, the three kinds,
    Gaussian rows and rows of a tone under a mean a thousand times its amplitude: the row bounds of the GPU tests hold"""
    worst = [0.0, 0.0]
    for n in (512, 8192):
        rng = np.random.default_rng(232 + n)
        j = np.arange(n)
        tones = (1000.0 + np.cos(2 * np.pi * np.outer([3, n // 4, n // 2 - 1], j) / n + 0.3)).astype(np.float32)
        for what, x in (("Gaussian", _rows(rng, (3, n))), ("tone + 1000 DC", tones)):
            for kind in KINDS:
                l2, mx = hm.errors(hm.chain(x, kind, np.float32), hm.chain(x, kind), x)
                print(f"n={n} kind {kind} {what}: fp32 model relL2 = {l2:.2e}, max = {mx:.2e}")
                worst = [max(worst[0], l2), max(worst[1], mx)]
                assert l2 <= ROW_REL_L2 and mx <= ROW_MAX, (n, kind, what, l2, mx)
    print(f"fp32 model, worst: relL2 = {worst[0]:.2e}, max |d| / max |x| = {worst[1]:.2e}")
    assert ROW_REL_L2 == 1e-6 and ROW_MAX == 5e-6


# ---- 2: ISA budget and inventory -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """{M: assembly of smfft_hilbert_<M>.o as the Makefile compiles it}"""
    if not os.path.exists(ac.HIPCC):
        pytest.skip("hipcc not installed")
    return ac.addon_isa("smfft_hilbert", "HILBERT", SIZES, tmp_path_factory.mktemp("hilbert_isa"))


def test_isa_budget_of_what_ships(isa):
    """per M exactly the three kernels, read from the compiled object's metadata: no scratch, at most 256 VGPRs (two waves per SIMD),
    static LDS of 34,816 B (the transform region of 4096 points; at most 64 B more), no transcendentals, no packed f32 arithmetic.  A
    thread's sixteen 8-byte non-temporal row loads go out up front with no branch or barrier between the first and the last; the kinds
    that need x at the store keep it in registers (a build with -DSMFFT_HILBERT_KEEP_X=0 in the Makefile's flags loads it a second time
    behind the transforms, again sixteen loads in one run); and every store -- sixteen non-temporal ones of 8 bytes, of 16 bytes for the analytic kind -- comes
    behind the last load, which is what serves d_out == d_in for kinds 0 and 2"""
    total = 0
    for m, text in isa.items():
        flags = ac.makefile_flags("HILBERT", m)
        assert "-ffp-contract=on" in flags, m
        keep = "-DSMFFT_HILBERT_KEEP_X=0" not in flags          # (kept is the default of smfft_hilbert.hip)
        descs = ac.descriptors(text)
        kernels = ac.pfb_kernels(text, "hilbert_kernel")
        assert len(descs) == 3 and set(descs) == set(kernels), (m, sorted(descs))
        total += len(descs)
        assert not re.search(r"\bscratch_", text), m
        for kind in KINDS:
            name = next(k for k in kernels if re.search(r"hilbert_kernelILi%dELi%dE" % (m, kind), k))
            body = kernels[name]
            assert not [line for line in body if re.match(r"v_(sin|cos)_", line)], name
            assert not [line for line in body if re.match(r"v_pk_(add|mul|fma)_f32", line)], name
            assert ac.descriptor_field(descs, name, "private_segment_fixed_size") == 0, name
            v, lds = ac.descriptor_field(descs, name, "next_free_vgpr"), ac.descriptor_field(descs, name, "group_segment_fixed_size")
            print(f"M={m}: hilbert_kernel<{m}, {kind}> {v} VGPRs ({ac.occupancy(v)} waves per SIMD), {lds} B of LDS, 0 B of scratch")
            assert LDS_BUDGET <= lds <= LDS_BUDGET + 64 and 2 * lds <= ac.LDS_PER_CU, (name, lds)
            assert v <= 256 and ac.occupancy(v) >= 2, (name, v)
            # the row loads are the non-temporal ones (the others, plain, are twiddles)
            loads = [i for i, line in enumerate(body) if line.startswith("global_load") and re.search(r"\bnt\b", line)]
            every_load = [i for i, line in enumerate(body) if line.startswith("global_load")]
            stores = [i for i, line in enumerate(body) if line.startswith("global_store")]
            runs = 1 if kind == 0 or keep else 2
            assert len(loads) == 16 * runs and all(re.match(r"global_load_dwordx2\s", body[i]) for i in loads), (name, len(loads))
            # up front in the tile loop: nothing but address arithmetic between them, and no LDS access in front of the last
            assert [i for i in every_load if loads[0] <= i <= loads[15]] == loads[:16], name
            label = max(i for i, line in enumerate(body[:loads[0]]) if re.match(r"\.LBB\d+_\d+:", line))
            assert not [line for line in body[label:loads[15]] if line.startswith(("ds_", "s_barrier"))], name
            for run in range(runs):
                between = body[loads[16 * run]:loads[16 * run + 15] + 1]
                assert not [line for line in between if line.startswith(("s_cbranch", "s_branch", "s_setpc", "s_barrier", "ds_"))], (name, run)
            assert len(stores) == 16, (name, len(stores))
            assert all(re.match(r"global_store_dwordx4\s" if kind == 1 else r"global_store_dwordx2\s", body[i])
                       and re.search(r"\bnt\b", body[i]) for i in stores), name
            assert min(stores) > max(every_load), name
    assert total == 15


def test_library_ships_fifteen_kernels_and_the_inventory_names_them(hilbert_lib):
    ac.check_inventory(hilbert_lib, hilbert_inventory.KERNELS, "smfft_hilbert_", 15, kinds=("tests", "bounds", "probes"))
    assert "permlane" in hilbert_inventory.__doc__ and "hostsim" in hilbert_inventory.__doc__


def test_isa_identity_compares_the_library():
    """tools/isa_identity.py compiles the five objects with the Makefile's flags and -I., like the other add-ons' (the tool itself
    needs the history of a git checkout and minutes of compiling: it is run by hand, DESIGN.md section 23 has its verdict)"""
    ac.check_isa_identity_lists("smfft_hilbert", "HILBERT", SIZES)


# ---- 3: declarations and exports ---------------------------------------------------------------------------------
def test_python_mirror_matches_header(hilbert_lib):
    from smfft_amd import hilbert
    text = open(os.path.join(ROOT, "include", "smfft_hilbert.h")).read()
    header = re.sub(r"[\s*]+", " ", text)
    for phrase in ("With X = DFT_n(x)", "H(x) = IDFT_n(-i s[k] X[k])", "s[k] = +1 for 0 < k < n/2, -1 for n/2 < k < n, 0 at k = 0 and k = n/2",
                   "exactly scipy.signal.hilbert(x).imag", "a = x + i H(x)", "The real part is the input to the bit; scipy's is only close to it",
                   "sqrt(x^2 + H(x)^2)", "z[p] = x[2p] + i x[2p+1]", "P[k] = conj Z[(M-k) mod M]",
                   "Z'[k] = (conj(W_n^k) (Z[k] + P[k]) - W_n^k (Z[k] - P[k])) / n, Z'[0] = 0", "W_n = exp(-2 pi i / n)",
                   "H(x)[2p] = Re z'[p] and H(x)[2p+1] = Im z'[p]", "1/n is a power of two and exact",
                   "In place, d_out == d_in, is allowed for kinds 0 and 2", "Ranges that overlap without being equal are refused",
                   "any overlap for kind 1", "every output element is written exactly once",
                   "the bits of row r's outputs depend only on x[r], n and kind", "A NaN or Inf in a row stays in that row",
                   "batch == 0 launches nothing and returns 0", "Out of scope", "n < 512, n > 8192 and n that is not a power of two",
                   "complex input", "a user-supplied frequency response", "instantaneous phase or frequency", "orthonormal scaling",
                   "two-dimensional transforms"):
        assert phrase in header, phrase
    values = dict(re.findall(r"#define (SMFFT_HILBERT_[A-Z]+) (\d+)", text))
    assert values == {"SMFFT_HILBERT_QUADRATURE": "0", "SMFFT_HILBERT_ANALYTIC": "1", "SMFFT_HILBERT_ENVELOPE": "2"}
    assert (hilbert.QUADRATURE, hilbert.ANALYTIC, hilbert.ENVELOPE) == (0, 1, 2) == hilbert.KINDS
    decl = ac.declarations("smfft_hilbert.h")
    assert sorted(decl) == sorted(hilbert.SIGS) == sorted(NAMES)
    for name, (res, args) in decl.items():
        assert hilbert.SIGS[name] == ac.signature(res, args), name
    assert hilbert.SIZES == SIZES and hilbert.LENGTHS == LENGTHS


def test_library_exports_exactly_the_four_symbols(hilbert_lib):
    ac.check_exports(hilbert_lib, NAMES)


# ---- 4: rejections -------------------------------------------------------------------------------------------------
def test_unsupported_combinations_return_minus_one_without_a_device(hilbert_lib):
    """-1 (or 0 for an empty batch) before any HIP call: run in a process where no GPU is visible, with null and bogus addresses that
    are never read.  Every length next to the five, kinds outside 0 ... 2, batch < 0, grid < 1, overlapping unequal buffers -- against
    the output's batch n 4 bytes, 8 for the analytic kind -- and the analytic kind in place"""
    code = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
ll, d, vp, i = ctypes.c_longlong, ctypes.c_double, ctypes.c_void_p, ctypes.c_int
head = [vp, vp, i, ll, i]
lib.smfft_hilbert_launch.argtypes = head + [vp]
lib.smfft_hilbert_launch_tuned.argtypes = head + [vp, i]
lib.smfft_hilbert_benchmark.argtypes = head + [ctypes.POINTER(d)]
t = d(0.0)
IN, OUT = 1 << 20, 1 << 30
def calls(n, batch, kind, grid=3, din=IN, dout=OUT):
    return [lib.smfft_hilbert_launch(din, dout, n, batch, kind, None),
            lib.smfft_hilbert_launch_tuned(din, dout, n, batch, kind, None, grid),
            lib.smfft_hilbert_benchmark(din, dout, n, batch, kind, ctypes.byref(t))]
rc = []
for n in (256, 500, 16384, 0, -512, 513, 1000, 8191, 2**31 - 1):
    for kind in (0, 1, 2):
        rc += calls(n, 10, kind) + calls(n, 0, kind) + calls(n, 10, kind, dout=IN) + calls(n, 10, kind, din=None, dout=None)
    rc += [lib.smfft_hilbert_fft_size(n)]
for n in (512, 8192):
    for kind in (3, -1, 4, 2**31 - 1):
        rc += calls(n, 10, kind) + calls(n, 0, kind)
    for kind in (0, 1, 2):
        rc += calls(n, -1, kind) + calls(n, -2**40, kind)
        size = 8 if kind == 1 else 4
        # overlapping, unequal: the output starts inside the input, or ends inside it, or one element off
        for off in (4, 4 * n, 4 * (10 * n - 1), -4, -(size * 10 * n - 4)):
            rc += calls(n, 10, kind, dout=IN + off)
        for grid in (0, -1):
            rc += [lib.smfft_hilbert_launch_tuned(IN, OUT, n, batch, kind, None, grid) for batch in (10, 0)]
    rc += calls(n, 10, 1, dout=IN)                                          # the analytic kind in place
    rc += calls(n, 10, 1, dout=IN - 8 * 10 * n + 4)                          # its output, twice the input, ends inside the input
empty = []
for n in (512, 1024, 2048, 4096, 8192):
    for kind in (0, 1, 2):
        empty += calls(n, 0, kind) + calls(n, 0, kind, dout=IN) + calls(n, 0, kind, dout=IN + 4) + calls(n, 0, kind, din=None, dout=None)
sizes = [lib.smfft_hilbert_fft_size(n) for n in (512, 1024, 2048, 4096, 8192)]
print(rc, empty, t.value, sizes)
ok = rc and rc == [-1] * len(rc) and empty == [0] * 180 and t.value == 0.0 and sizes == [256, 512, 1024, 2048, 4096]
sys.exit(0 if ok else 1)
"""
    p = subprocess.run([sys.executable, "-c", code, hilbert_lib], capture_output=True, text=True, timeout=120, env=dict(os.environ, **NO_DEVICE))
    assert p.returncode == 0, p.stdout + p.stderr


def test_python_wrappers_refuse_before_a_device(hilbert_lib):
    """in a process where no GPU is visible: the pointer forms turn the library's -1 into a RuntimeError, the array forms raise
    ValueError or TypeError themselves, and an empty batch is served"""
    code = ac.REFUSED + r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from smfft_amd import hilbert as hb
IN, OUT = 1 << 20, 1 << 30
for n in (256, 500, 16384, 0):
    refused(RuntimeError, hb.launch_ptr, IN, OUT, n, 10)
    refused(RuntimeError, hb.launch_tuned, IN, OUT, n, 10, 3)
    assert hb.benchmark(IN, OUT, n, 10) == (-1, 0.0)
    refused(ValueError, hb.fft_size, n)
    refused(ValueError, hb.hilbert, np.zeros((2, n), np.float32))
    refused(ValueError, hb.analytic, np.zeros((2, n), np.float32))
    refused(ValueError, hb.envelope, np.zeros((2, n), np.float32))
for kind in (3, -1):
    refused(RuntimeError, hb.launch_ptr, IN, OUT, 512, 10, kind)
refused(RuntimeError, hb.launch_ptr, IN, OUT, 512, -1)
refused(RuntimeError, hb.launch_ptr, IN, IN + 4, 512, 10)
refused(RuntimeError, hb.launch_ptr, IN, IN, 512, 10, hb.ANALYTIC)
refused(RuntimeError, hb.launch_tuned, IN, OUT, 512, 10, 0)
refused(TypeError, hb.hilbert, np.zeros((2, 512), np.complex64))
refused(ValueError, hb.hilbert, np.float32(1))
refused(TypeError, hb.launch, np.zeros((2, 512), np.float32))
import torch
refused(ValueError, hb.launch, torch.zeros(2, 512))                     # a tensor on the host: no CPU fallback
refused(ValueError, hb.launch, torch.zeros(2, 500))
refused(TypeError, hb.launch, torch.zeros(2, 512, dtype=torch.float64))
refused(ValueError, hb.launch, torch.zeros(2, 1024)[:, ::2])
refused(ValueError, hb.launch, torch.zeros(2, 512), kind=3)
refused(TypeError, hb.launch, torch.zeros(2, 512), torch.zeros(2, 512), kind=hb.ANALYTIC)                 # a float32 out for complex64
refused(TypeError, hb.launch, torch.zeros(2, 512), torch.zeros(2, 512, dtype=torch.complex64), kind=hb.ENVELOPE)
refused(ValueError, hb.launch, torch.zeros(2, 512), torch.zeros(2, 1024))
hb.launch_ptr(IN, IN, 8192, 0, hb.ENVELOPE)                              # an empty batch, in place: nothing is launched
assert hb.benchmark(IN, OUT, 512, 0) == (0, 0.0) and hb.fft_size(8192) == 4096
print("ok")
"""
    p = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300, env=dict(os.environ, **NO_DEVICE))
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout + p.stderr


def test_import_does_not_load_the_library():
    ac.check_import_does_not_load("hilbert", "smfft_hilbert")

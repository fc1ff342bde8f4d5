"""The polyphase filter bank channelizer for real streams (smfft_amd/csrc/smfft_pfb_real.hip, include/smfft_pfb_real.h) on the CPU: the
fp64 model's two forms of the definition agree, with one tap of ones it is np.fft.rfft, and it equals channels 0 ... N of the complex
bank's model at 2N channels; the gfx950 code keeps the library's rules (no scratch, no v_sin / v_cos, no packed f32, the VGPRs of three
workgroups per compute unit, the sixteen signal loads of a tap together); the C ABI declares, exports and validates without a device; every shipped kernel is in tests/pfb_inventory.py with its tests.
No GPU code is run (hipcc cross-compiles gfx950)."""
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

from tests import addon_checks as ac  # noqa: E402
from tests import pfb_inventory as pinv  # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "smfft_amd", "csrc")
SRC = os.path.join(CSRC, "smfft_pfb_real.hip")
SIZES = (256, 512, 1024, 2048, 4096)
WORKGROUPS_PER_CU = 3      # kWorkgroupsPerCu of smfft_pfb_real.hip
VGPR_BUDGET = 168          # three waves per SIMD: 512 registers / 3, in granules of 8
LDS_PER_CU = 160 * 1024


# ------------------------------------------------------------------------------------------------ the model
def test_models_two_forms_agree():
    rng = np.random.default_rng(0)
    N = 256
    for P, C, L in ((1, 1, 512), (2, 2, 5 * 512 + 18), (4, 1, 7 * 512 + 510), (32, 1, 34 * 512 + 2)):
        x, h = rng.standard_normal((C, L)), rng.standard_normal(P * 2 * N)
        a, b = prm.pfb_real(x, h, N), prm.pfb_real_direct(x, h, N)
        assert a.shape == (C, L // (2 * N) - P + 1, N + 1)
        assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b)), (P, C, L)
        # packing and power: element 0 holds DC and Nyquist / the DC power, the others are the spectrum's
        p, w = prm.pack(a), prm.power(a)
        assert p.shape == w.shape == a.shape[:-1] + (N,)
        assert np.array_equal(p[..., 1:], a[..., 1:N]) and np.array_equal(p[..., 0].real, a[..., 0].real)
        assert np.array_equal(p[..., 0].imag, a[..., N].real)
        assert np.allclose(w, np.abs(a[..., :N]) ** 2, rtol=1e-12)
        assert np.max(np.abs(a[..., 0].imag)) <= 1e-9 * np.max(np.abs(a)) and np.max(np.abs(a[..., N].imag)) <= 1e-9 * np.max(np.abs(a))


@pytest.mark.parametrize("N", [256, 1024, 4096])
def test_model_with_one_tap_of_ones_is_the_plain_rfft(N):
    rng = np.random.default_rng(N)
    x = rng.standard_normal((2, 5 * 2 * N + 12))
    want = np.fft.rfft(x[:, :5 * 2 * N].reshape(2, 5, 2 * N), axis=-1)
    got = prm.pfb_real(x, np.ones(2 * N), N)
    assert got.shape == want.shape == (2, 5, N + 1)
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))


@pytest.mark.parametrize("N", SIZES)
def test_model_is_the_lower_half_of_the_complex_banks_model(N):
    """channels 0 ... N of pfb_model.pfb(x + 0j, h, 2N): the new definition is the shipped one on a real signal"""
    rng = np.random.default_rng(7 * N)
    for P, C, tail in ((1, 1, 0), (3, 2, 2 * N - 2), (8, 1, 6)):
        L = (P + 2) * 2 * N + tail
        x, h = rng.standard_normal((C, L)), rng.standard_normal(P * 2 * N)
        want = pm.pfb(x + 0j, h, 2 * N)
        got = prm.pfb_real(x, h, N)
        assert got.shape == (C, 3, N + 1) and want.shape == (C, 3, 2 * N)
        assert prm.frames(L, N, P) == pm.frames(L, 2 * N, P) == pm.Plan(L // 2, N, P, C).frames() == 3
        assert np.max(np.abs(got - want[..., :N + 1])) <= 1e-12 * np.max(np.abs(want)), (N, P)
        assert np.allclose(prm.scale(x, h, N), pm.scale(x, h, 2 * N), rtol=1e-13)


# ------------------------------------------------------------------------------------------------ gfx950 code
@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """smfft_pfb_real_<N>.o as the Makefile compiles it: -I. and PFB_REAL_FLAGS_<N>"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    tmp = tmp_path_factory.mktemp("pfb_real_isa")

    def compile_one(n):
        return ac.device_asm(SRC, ["-I" + CSRC] + ac.makefile_flags("PFB_REAL", n) + [f"-DSMFFT_PFB_REAL_N={n}"], tmp / f"pfb_real_{n}.s")
    with concurrent.futures.ThreadPoolExecutor(len(SIZES)) as pool:
        return dict(zip(SIZES, pool.map(compile_one, SIZES)))


def _kernels(text):
    found = {}
    for m in re.finditer(r"^(_Z\w*pfb_real_kernel\w*):[^\n]*\n(.*?)\n\s*s_endpgm", text, re.S | re.M):
        found[m.group(1)] = [line.strip() for line in m.group(2).split("\n")]
    return found


def test_kernels_fit_three_workgroups_per_cu_without_scratch(isa):
    source = open(SRC).read()
    assert re.search(r"constexpr int kWorkgroupsPerCu = %d;" % WORKGROUPS_PER_CU, source)
    total = 0
    for n, text in isa.items():
        kernels = _kernels(text)
        descs = ac.descriptors(text)
        assert len(kernels) == 2 and len(descs) == 2, (n, sorted(kernels), sorted(descs))          # complex and power, nothing else
        total += len(kernels)
        for name, body in kernels.items():
            assert "pfb_real_kernelILi%dE" % n in name
            assert not [line for line in body if line.startswith("scratch_")], name
            assert not [line for line in body if re.match(r"v_(sin|cos)_", line)], name
            assert not [line for line in body if re.match(r"v_pk_\w+_f32", line)], name
            assert ac.descriptor_field(descs, name, "private_segment_fixed_size") == 0, name
            vgprs, lds = ac.descriptor_field(descs, name, "next_free_vgpr"), ac.descriptor_field(descs, name, "group_segment_fixed_size")
            print(f"N={n:5d} {'power  ' if 'ELi1EEE' in name else 'complex'}: {vgprs} VGPRs, {lds} B of LDS")
            assert lds == 4096 // 16 * 17 * 8 and WORKGROUPS_PER_CU * lds <= LDS_PER_CU, name
            assert vgprs <= VGPR_BUDGET, (name, vgprs)
    assert total == 10


def test_signal_loads_of_a_tap_are_issued_together(isa):
    """the sixteen signal loads of one tap (the kernel's only non-temporal loads) are contiguous in the instruction stream up to
    address arithmetic, with no branch, barrier or vmcnt(0) between the first and the last, and sit in a loop (a backward branch
    follows them); its sixteen coefficient pairs -- plain 8-byte loads -- follow them inside the loop"""
    arithmetic = re.compile(r"(v_add|v_addc|v_lshl|v_lshlrev|v_mov|v_mad|v_ashr|v_and|v_or|s_add|s_addc|s_lshl|s_mov|s_nop|s_mul|s_waitcnt lgkmcnt|;)")
    for n, text in isa.items():
        for name, body in _kernels(text).items():
            loads = [i for i, line in enumerate(body) if re.match(r"global_load_dwordx2 v\[\d+:\d+\], v\[\d+:\d+\], off( offset:-?\d+)? nt$", line)]
            assert len(loads) == 16, (name, len(loads))
            assert len([line for line in body if line.startswith("global_load") and line.endswith(" nt")]) == 16, name
            between = body[loads[0]:loads[-1] + 1]
            assert not [line for line in between if line.startswith(("s_cbranch", "s_branch", "s_setpc", "s_barrier"))], name
            assert not [line for line in between if re.search(r"vmcnt\(0\)", line)], name
            others = [line for line in between if line and not line.startswith("global_load_dwordx2")]
            assert all(arithmetic.match(line) for line in others), (name, others)
            # the loop: the first label before the loads is the target of the first branch after them
            label = next(line for line in reversed(body[:loads[0]]) if re.match(r"\.LBB\d+_\d+:", line)).split(":")[0]
            branch = next(line for line in body[loads[-1]:] if line.startswith("s_cbranch"))
            assert branch.split()[-1] == label, (name, label, branch)
            end = body.index(branch, loads[-1])
            taps = [i for i in range(loads[-1] + 1, end) if re.match(r"global_load_dwordx2 v\[\d+:\d+\], v\[\d+:\d+\], off( offset:-?\d+)?$", body[i])]
            assert len(taps) == 16, (name, len(taps))


# ------------------------------------------------------------------------------------------------ C ABI
NAMES = ("smfft_pfb_real_frames", "smfft_pfb_real_launch", "smfft_pfb_real_benchmark", "smfft_pfb_real_launch_tuned",
         "smfft_pfb_real_default_tile_run")


@pytest.fixture(scope="module")
def pr():
    from smfft_amd import pfb_real
    pfb_real.lib()
    return pfb_real


def test_header_declarations_equal_the_ctypes_signatures(pr):
    from smfft_amd import pfb
    header = open(os.path.join(ROOT, "include", "smfft_pfb_real.h")).read()
    for phrase in ("Out of scope", "oversampled", "complex prototypes", "synthesis", "Nyquist power", "NOT output", "N <= 128", "N >= 8192", "EVEN"):
        assert phrase in header, phrase
    decl = ac.declarations("smfft_pfb_real.h")
    assert sorted(decl) == sorted(pr.SIGS) == sorted(NAMES)
    for name, (res, args) in decl.items():
        assert pr.SIGS[name] == ac.signature(res, args), name
    # one for one the complex bank's functions, in arguments and results
    for name in NAMES:
        assert pr.SIGS[name] == pfb.SIGS[name.replace("pfb_real", "pfb")], name
    assert pr.SIZES == SIZES
    # the complex bank's header points real input here
    assert "smfft_pfb_real.h" in open(os.path.join(ROOT, "include", "smfft_pfb.h")).read()


def test_library_exports_exactly_the_five_symbols(pr):
    nm = subprocess.run(["nm", "-D", "--defined-only", pr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r" T (smfft_\w+)$", nm, re.M)) == sorted(NAMES)


def test_unsupported_combinations_return_minus_one_without_a_device(pr):
    """all validation happens before any HIP call: these return -1 (or 0 when there is no whole frame) with no device and null pointers"""
    lib = pr.lib()
    t = ctypes.c_double(0.0)
    bad = [(1 << 20, 1, n, 4) for n in (0, 128, 1000, 8192, -1024)] + [(1 << 20, 1, 1024, p) for p in (0, 33, -1)]
    bad += [(1 << 20, c, 1024, 4) for c in (0, -1)] + [(-2, 1, 1024, 4), (-1, 1, 1024, 4)]
    bad += [((1 << 20) + 1, 1, 1024, 4), (8 * 2048 + 1, 2, 1024, 4), (1, 1, 256, 1), (3, 1, 1024, 4)]      # odd lengths
    for L, C, N, P in bad:
        for power in (0, 1):
            assert lib.smfft_pfb_real_launch(None, L, C, None, N, P, power, None, None) == -1, (L, C, N, P)
            assert lib.smfft_pfb_real_launch_tuned(None, L, C, None, N, P, power, None, None, 3) == -1, (L, C, N, P)
            assert lib.smfft_pfb_real_benchmark(None, L, C, None, N, P, power, None, ctypes.byref(t)) == -1, (L, C, N, P)
    assert lib.smfft_pfb_real_launch_tuned(None, 1 << 20, 1, None, 1024, 4, 0, None, None, -1) == -1
    # no whole frame is not an error: nothing is launched
    for L in (0, 2046, 4 * 2048 - 2):
        for power in (0, 1):
            assert lib.smfft_pfb_real_launch(None, L, 2, None, 1024, 4, power, None, None) == 0
            assert lib.smfft_pfb_real_launch_tuned(None, L, 2, None, 1024, 4, power, None, None, 7) == 0
            assert lib.smfft_pfb_real_benchmark(None, L, 2, None, 1024, 4, power, None, ctypes.byref(t)) == 0
    assert t.value == 0.0
    for n in (0, 128, 1000, 8192):
        assert lib.smfft_pfb_real_frames(1 << 20, n, 4) == -1 and lib.smfft_pfb_real_default_tile_run(n, 4) == -1
    for p in (0, 33, -1):
        assert lib.smfft_pfb_real_frames(1 << 20, 1024, p) == -1 and lib.smfft_pfb_real_default_tile_run(1024, p) == -1
    assert lib.smfft_pfb_real_frames(-2, 1024, 4) == -1 and lib.smfft_pfb_real_frames((1 << 20) + 1, 1024, 4) == -1
    with pytest.raises(ValueError):
        pr.frames(1000, 100, 4)
    with pytest.raises(ValueError):
        pr.frames(8 * 2048 + 1, 1024, 4)
    with pytest.raises(RuntimeError):
        pr.launch(None, 1 << 20, 1, None, 8192, 4, None)
    with pytest.raises(ValueError):
        pr.channelize(np.zeros(4096, np.float32), np.zeros(100, np.float32), 256)
    with pytest.raises(ValueError):
        pr.channelize(np.zeros(4096, np.complex64), np.zeros(512, np.float32), 256)
    assert pr.channelize(np.zeros((2, 1000), np.float32), np.zeros(1024, np.float32), 256).shape == (2, 0, 257)
    assert pr.channelize(np.zeros((2, 1000), np.float32), np.zeros(1024, np.float32), 256, packed=True).shape == (2, 0, 256)
    assert pr.channelize(np.zeros((2, 1000), np.float32), np.zeros(1024, np.float32), 256, power=True).shape == (2, 0, 256)


def test_every_pfb_real_kernel_is_in_the_inventory_with_its_tests(pr):
    """the rule of tests/test_kernel_inventory.py, without the "host" kind (tests/pfb_inventory.py says why)"""
    ac.check_inventory(pr.LIB_PATH, pinv.REAL_KERNELS, "smfft_pfb_real_", 10, kinds=("tests", "bounds", "probes"))


def test_frames_over_ragged_lengths_and_default_tile_run(pr):
    for N in SIZES:
        for P in (1, 4, 32):
            assert pr.default_tile_run(N, P) >= 1
            for L in (0, 2 * N - 2, 2 * P * N - 2, 2 * P * N, 2 * P * N + 2, (P + 9) * 2 * N + 2 * N - 2, (1 << 34) + 6):
                assert pr.frames(L, N, P) == max(L // (2 * N) - P + 1, 0) == prm.frames(L, N, P) == pm.frames(L // 2, N, P)


def test_prototype(pr):
    for N, P in ((256, 1), (256, 4), (1024, 8), (4096, 32), (512, 3)):
        h = pr.prototype(N, P)
        M = 2 * P * N
        assert h.dtype == np.float32 and h.shape == (M,)
        assert np.array_equal(h, h[::-1]), "symmetric to the bit"
        assert h[M // 2 - 1] == h[M // 2] == h.max()
        m = np.arange(M, dtype=np.float64)
        want = np.sinc((m - (M - 1) / 2) / (2 * N)) * (0.54 - 0.46 * np.cos(2 * np.pi * m / (M - 1)))
        assert np.array_equal(h, want.astype(np.float32)) or np.max(np.abs(h.astype(np.float64) - want)) <= 2.0 ** -24 * np.max(np.abs(want))
    assert np.array_equal(pr.prototype(256, 2, "rectangular"), np.sinc((np.arange(1024) - 511.5) / 512).astype(np.float32))
    with pytest.raises(ValueError):
        pr.prototype(256, 2, "kaiser")
    # unpack: the device's rows -> np.fft.rfft layout
    rows = (np.arange(12) + 1j * np.arange(12, 24)).reshape(3, 4).astype(np.complex64)
    un = pr.unpack(rows)
    assert un.shape == (3, 5) and np.array_equal(un[:, 1:4], rows[:, 1:]) and np.array_equal(un[:, 0], rows[:, 0].real) and np.array_equal(un[:, 4], rows[:, 0].imag)

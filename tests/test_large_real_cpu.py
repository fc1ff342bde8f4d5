"""CPU checks of the real N = 16384 / 32768 single-pass R2C / C2R (include/smfft/smfft_large_real.hpp, libsmfft_large_real.so): the
fp64 model of the split / merge on the engine's layout (tools/large_real_model.py) against numpy and its LDS bank conflicts, the
header's twiddle rows against fp64 through a host compile and the committed W_32768 row against its generator, the ISA budgets of
both objects, the -1 cases without a device, the Python mirror of include/smfft_large_real.h, and the kernel inventory of the library
(tests/large_real_inventory.py)."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_twiddles_32768  # noqa: E402
import large_plan_model as lpm  # noqa: E402
import large_real_model as lrm  # noqa: E402

from oracle import np_reference as ref  # noqa: E402
from tests import addon_checks as ac  # noqa: E402
from tests import large_real_inventory as rinv  # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "smfft_amd", "csrc")
LIB = os.path.join(ROOT, "smfft_amd", "libsmfft_large_real.so")
SIZES = (16384, 32768)
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def real_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", CSRC, "-j", "4", "../libsmfft_large_real.so"])
    return LIB


# ---- the model -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_model_r2c_is_rfft(n):
    x = np.random.default_rng(n).standard_normal(n)
    got = lrm.r2c(x)
    full = np.fft.rfft(x)
    assert np.linalg.norm(got[1:] - full[1:n // 2]) / np.linalg.norm(full) < 1e-14
    assert abs(got[0] - complex(full[0].real, full[n // 2].real)) < 1e-12 * np.abs(full).max()
    assert np.allclose(got, ref.r2c_packed(x[None])[0], rtol=0, atol=1e-12 * np.abs(full).max())


@pytest.mark.parametrize("n", SIZES)
def test_model_c2r_is_c2r_packed(n):
    rng = np.random.default_rng(n + 1)
    xp = rng.standard_normal(n // 2) + 1j * rng.standard_normal(n // 2)
    got = lrm.c2r(xp)
    want = ref.c2r_packed(xp[None])[0]
    assert np.linalg.norm(got - want) / np.linalg.norm(want) < 1e-14
    # and the round trip of the model: C2R(R2C(x)) = (N/2) x
    x = rng.standard_normal(n)
    assert np.linalg.norm(lrm.c2r(lrm.r2c(x)) - (n / 2) * x) / np.linalg.norm((n / 2) * x) < 1e-14


@pytest.mark.parametrize("n", SIZES)
def test_exchange_s_is_conflict_free(n):
    c = lpm.Conflicts()
    lrm.r2c(np.ones(n), c)
    lrm.c2r(np.ones(n // 2, dtype=complex), c)
    ratios = c.ratio()
    assert set(ratios) == {("S write", "w"), ("S read", "r")}
    assert all(v == 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("n", SIZES)
def test_lds_budget(n):
    g = lrm.geometry(n)
    nbytes = 8 * g["LDS_FLOAT2"]
    assert g["LDS_FLOAT2"] > g["L"]            # room for element 0's second copy at L
    assert nbytes <= (81920 if n == 16384 else 163840)


# ---- the header through a host compile -------------------------------------------------------------
def _host_run(tmp_path, body):
    src = tmp_path / "large_real_host.hip"
    src.write_text('#include <cstdio>\n#include "smfft/smfft_large_real.hpp"\nint main() {\n' + body + "\n    return 0;\n}\n")
    exe = tmp_path / "large_real_host"
    subprocess.check_call([HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                          stderr=subprocess.DEVNULL)
    return subprocess.check_output([str(exe)], text=True)


def _within_half_ulp(got, exact):
    for g, v in zip(got.reshape(-1), exact.reshape(-1)):
        if abs(v) < 1e-12:
            assert g == 0.0, (g, v)
        else:
            assert abs(g - v) <= 2.0 ** (math.frexp(abs(v))[1] - 25), (g, v)


@needs_hipcc
def test_header_split_rows_are_correctly_rounded(tmp_path):
    """v[u] = -(i/2) W_N^u (R2C) and (i/2) conj W_N^u (C2R), u < N/32, within 0.5 ulp of fp64; w32[q] = W_32^{+-q} the exact entries
    of the W_16384 table; the geometry and the partner slots of the model"""
    body = ""
    for n in SIZES:
        for d in (0, 1):
            body += (f"    {{ constexpr smfft::large::LargeRealTwiddles<{n}, {d}> r; for (auto w : r.v) printf(\"%a %a\\n\", w.x, w.y); "
                     f"for (auto w : r.w32) printf(\"%a %a\\n\", w.x, w.y); }}\n")
        body += (f"    {{ using RG = smfft::large::LargeRealGeometry<{n}>; printf(\"%d %d %d\\n\", RG::L, RG::T, RG::G::kLdsFloat2);\n"
                 f"      for (int p = 0; p < RG::L; ++p) printf(\"%d %d\\n\", RG::partner(p), RG::partner_slot(p)); }}\n")
    lines = _host_run(tmp_path, body).strip().split("\n")
    pos = 0
    for n in SIZES:
        T = n // 32
        for d in (0, 1):
            vals = np.array([[float.fromhex(a) for a in line.split()] for line in lines[pos:pos + T + 16]])
            pos += T + 16
            vu, w32 = lrm.split_rows(n, bool(d))
            _within_half_ulp(vals[:T, 0], vu.real)
            _within_half_ulp(vals[:T, 1], vu.imag)
            # W_32^q are W_16384^{512 q}: correctly rounded, exact at q = 0 and 8, symmetric about q = 4
            _within_half_ulp(vals[T:, 0], w32.real)
            _within_half_ulp(vals[T:, 1], w32.imag)
            assert tuple(vals[T]) == (1.0, 0.0) and tuple(vals[T + 8]) == (0.0, 1.0 if d else -1.0)
            assert np.array_equal(np.abs(vals[T + 4]), np.abs(vals[T + 12][::-1]))
        L, Tg, lds = (int(v) for v in lines[pos].split())
        g = lrm.geometry(n)
        assert (L, Tg, lds) == (g["L"], g["T"], g["LDS_FLOAT2"])
        pairs = np.array([[int(v) for v in line.split()] for line in lines[pos + 1:pos + 1 + L]])
        p = np.arange(L)
        assert np.array_equal(pairs[:, 0], (L - p) % L) and np.array_equal(pairs[:, 1], L - p)
        pos += 1 + L
    assert pos == len(lines)


def test_committed_row_is_the_generators_output():
    path = os.path.join(ROOT, "include", "smfft", "smfft_twiddles_32768.inc")
    assert os.path.abspath(gen_twiddles_32768.PATH) == os.path.abspath(path)
    assert open(path).read() == gen_twiddles_32768.table_text()
    c, s = gen_twiddles_32768.row()
    ang = 2 * np.pi * np.arange(1024) / 32768
    _within_half_ulp(c.astype(np.float64), np.cos(ang))
    _within_half_ulp(s.astype(np.float64), np.sin(ang))


# ---- ISA of what ships -------------------------------------------------------------------------------
@needs_hipcc
@pytest.mark.parametrize("n", SIZES)
def test_isa_budget(tmp_path, n):
    text = ac.device_asm(os.path.join(CSRC, "smfft_large_real.hip"), ac.makefile_flags("LARGE_REAL", n) + [f"-DSMFFT_LARGE_REAL_N={n}"],
                         tmp_path / f"large_real_{n}.s")
    kernels = ac.descriptors(text)
    assert sorted(kernels) == sorted([f"_ZN5smfft5large9large_c2rILi{n}EEEvPK15HIP_vector_typeIfLj2EEPfi",
                                                    f"_ZN5smfft5large9large_r2cILi{n}EEEvPKfP15HIP_vector_typeIfLj2EEi"])
    for name in kernels:
        assert ac.descriptor_field(kernels, name, "private_segment_fixed_size") == 0, name
        lds = ac.descriptor_field(kernels, name, "group_segment_fixed_size")
        assert lds <= (81920 if n == 16384 else 163840), (name, lds)
        assert ac.descriptor_field(kernels, name, "next_free_vgpr") <= 128, name
    assert not re.search(r"\bv_(sin|cos)_", text)
    assert not re.search(r"\bv_pk_(add|mul|fma)_f32", text)
    assert not re.search(r"\bscratch_", text)


# ---- C ABI and Python mirror ---------------------------------------------------------------------------
def test_python_mirror_matches_header(real_lib):
    from smfft_amd import large_real
    decl = ac.declarations("smfft_large_real.h")
    assert sorted(decl) == sorted(large_real.SIGS) == ["smfft_large_real_benchmark", "smfft_large_real_grid", "smfft_large_real_launch"]
    for name, (res, args) in decl.items():
        assert res == "int" and large_real.SIGS[name] == ac.signature(res, args), name
    assert large_real.SIZES == SIZES
    lib = ctypes.CDLL(real_lib)
    for name in decl:
        assert hasattr(lib, name), name


def test_unsupported_calls_return_minus_one_without_a_device(real_lib):
    """-1 before any HIP call: run in a process where no GPU is visible, with null pointers"""
    code = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
t = ctypes.c_double(0.0)
cases = ((8192, 1), (16383, 1), (65536, 1), (0, 1), (16384, -1), (32768, -5))
rc = [lib.smfft_large_real_launch(None, None, n, c, d, None) for n, c in cases for d in (0, 1)]
rc += [lib.smfft_large_real_benchmark(None, None, n, c, d, ctypes.byref(t)) for n, c in cases for d in (0, 1)]
rc += [lib.smfft_large_real_grid(4096), lib.smfft_large_real_grid(8192), lib.smfft_large_real_grid(65536)]
print(rc, t.value)
sys.exit(0 if rc == [-1] * 27 and t.value == 0.0 else 1)
"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code, real_lib], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stdout + p.stderr


def test_host_helpers_reject_other_lengths():
    from smfft_amd import large_real
    with pytest.raises(ValueError):
        large_real.r2c(np.zeros((1, 8192), np.float32))
    with pytest.raises(ValueError):
        large_real.c2r(np.zeros((1, 4096), np.complex64))


def test_import_does_not_load_the_large_real_library():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import smfft_amd, smfft_amd.large_real as l; assert l._lib is None; "
            "import os; maps = open('/proc/self/maps').read(); assert 'libsmfft_large_real' not in maps; print('ok')")
    p = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout + p.stderr


# ---- kernel inventory of libsmfft_large_real.so -----------------------------------------------------------
def test_every_large_real_kernel_is_in_the_inventory_with_its_tests(real_lib):
    ac.check_inventory(real_lib, rinv.KERNELS, "smfft_large_real_", 4)

"""CPU checks of the N = 8192 / 16384 single-pass C2C engine (include/smfft/smfft_large.hpp, libsmfft_large.so): the fp64 model of
the plan (tools/large_plan_model.py) against numpy.fft and its LDS bank conflicts, the header's constants and twiddle table against
the model and fp64 through a host compile, the ISA budgets of both objects, the -1 cases without a device, the Python mirror of
include/smfft_large.h, and the kernel inventory of the library (tests/large_inventory.py)."""
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
import gen_twiddles_16384  # noqa: E402
import large_plan_model as lpm  # noqa: E402

from tests import addon_checks as ac  # noqa: E402
from tests import large_inventory as linv  # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "smfft_amd", "csrc")
LIB = os.path.join(ROOT, "smfft_amd", "libsmfft_large.so")
SIZES = (8192, 16384)
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def large_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", CSRC, "-j", "4", "../libsmfft_large.so"])
    return LIB


# ---- the plan ------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", (False, True))
@pytest.mark.parametrize("n", SIZES)
def test_plan_model_is_the_dft(n, inverse):
    rng = np.random.default_rng(n + inverse)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    want = np.fft.ifft(x) * n if inverse else np.fft.fft(x)
    got = lpm.run(x, inverse)
    assert np.linalg.norm(got - want) / np.linalg.norm(want) < 1e-14


@pytest.mark.parametrize("n", SIZES)
def test_every_lds_access_is_conflict_free(n):
    c = lpm.Conflicts()
    lpm.run(np.ones(n, dtype=complex), False, c)
    ratios = c.ratio()
    assert {k[0] for k in ratios} == {"A write", "A read", "B write", "B read", "C write", "C read"}
    assert all(v == 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("n", SIZES)
def test_lds_budget(n):
    g = lpm.geometry(n)
    nbytes = 8 * g["LDS_FLOAT2"]
    assert nbytes <= 163840
    assert (163840 // nbytes) == (2 if n == 8192 else 1)


# ---- the header through a host compile -------------------------------------------------------------
def _host_run(tmp_path, body):
    src = tmp_path / "large_host.hip"
    src.write_text('#include <cstdio>\n#include "smfft/smfft_large.hpp"\nint main() {\n' + body + "\n    return 0;\n}\n")
    exe = tmp_path / "large_host"
    subprocess.check_call([HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                          stderr=subprocess.DEVNULL)
    return subprocess.check_output([str(exe)], text=True)


@needs_hipcc
def test_header_computes_the_models_constants(tmp_path):
    body = ""
    for n in SIZES:
        body += (f"    {{ using G = smfft::large::LargeGeometry<{n}>; printf(\"%d %d %d %d %d %d\\n\", G::T, G::R, G::SA, G::kLdsFloat2, "
                 f"G::kWorkgroupsPerCu, G::B3);\n      for (int p = 0; p < {n}; ++p) printf(\"%d\\n\", G::lds_a(p)); }}\n")
    out = _host_run(tmp_path, body).split("\n")
    pos = 0
    for n in SIZES:
        g = lpm.geometry(n)
        head = [int(v) for v in out[pos].split()]
        assert head == [g["T"], g["R"], g["SA"], g["LDS_FLOAT2"], 2 if n == 8192 else 1, 16 // g["R"]]
        got = np.array([int(v) for v in out[pos + 1:pos + 1 + n]])
        assert np.array_equal(got, lpm.lds_a(n, np.arange(n)))
        pos += 1 + n


@needs_hipcc
def test_header_twiddles_are_correctly_rounded(tmp_path):
    """every W_16384^m the header rebuilds from the octant is within 0.5 ulp of fp64, quarter turns exact, equal to the generator's
    expansion; and the per-N rows hold the exponents of the model"""
    body = "    for (int m = 0; m < 16384; ++m) { auto w = smfft::large::w16384(m); printf(\"%a %a\\n\", w.x, w.y); }\n"
    for n in SIZES:
        body += (f"    {{ constexpr smfft::large::LargeTwiddleRows<{n}> r; for (auto w : r.w2) printf(\"%a %a\\n\", w.x, w.y); "
                 f"for (auto w : r.w3) printf(\"%a %a\\n\", w.x, w.y); for (auto w : r.w4) printf(\"%a %a\\n\", w.x, w.y); }}\n")
    vals = np.array([[float.fromhex(a) for a in line.split()] for line in _host_run(tmp_path, body).strip().split("\n")])
    table = vals[:16384]
    assert np.array_equal(table, gen_twiddles_16384.full_table().astype(np.float64))
    ang = 2 * np.pi * np.arange(16384) / 16384
    exact = np.stack([np.cos(ang), -np.sin(ang)], axis=1)
    for m in range(16384):
        for j in range(2):
            v = exact[m, j]
            if abs(v) < 1e-12:
                assert table[m, j] == 0.0, (m, j)
            else:
                assert abs(table[m, j] - v) <= 2.0 ** (math.frexp(abs(v))[1] - 25), (m, j, table[m, j], v)
    for m, want in {0: (1.0, 0.0), 4096: (0.0, -1.0), 8192: (-1.0, 0.0), 12288: (0.0, 1.0)}.items():
        assert tuple(table[m]) == want
    pos = 16384
    for n in SIZES:
        exps = sum(lpm.twiddle_rows(n), [])
        rows = vals[pos:pos + len(exps)]
        assert np.array_equal(rows, table[exps])
        pos += len(exps)
    assert pos == len(vals)


def test_committed_octant_is_the_generators_output():
    path = os.path.join(ROOT, "include", "smfft", "smfft_twiddles_16384.inc")
    assert os.path.abspath(gen_twiddles_16384.PATH) == os.path.abspath(path)
    assert open(path).read() == gen_twiddles_16384.table_text()


# ---- ISA of what ships -------------------------------------------------------------------------------
@needs_hipcc
@pytest.mark.parametrize("n", SIZES)
def test_isa_budget(tmp_path, n):
    text = ac.device_asm(os.path.join(CSRC, "smfft_large.hip"), ac.makefile_flags("LARGE", n) + [f"-DSMFFT_LARGE_N={n}"], tmp_path / f"large_{n}.s")
    kernels = ac.descriptors(text)
    assert len(kernels) == 2
    for name in kernels:
        assert ac.descriptor_field(kernels, name, "private_segment_fixed_size") == 0, name
        lds = ac.descriptor_field(kernels, name, "group_segment_fixed_size")
        assert lds <= 163840 and (n != 8192 or lds <= 81920), (name, lds)
        assert ac.descriptor_field(kernels, name, "next_free_vgpr") <= 128, name
    assert not re.search(r"\bv_(sin|cos)_", text)
    assert not re.search(r"\bv_pk_(add|mul|fma)_f32", text)


# ---- C ABI and Python mirror ---------------------------------------------------------------------------
def test_python_mirror_matches_header(large_lib):
    from smfft_amd import large
    decl = ac.declarations("smfft_large.h")
    assert sorted(decl) == sorted(large.SIGS)
    for name, (res, args) in decl.items():
        assert res == "int" and large.SIGS[name] == ac.signature(res, args), name
    lib = ctypes.CDLL(large_lib)
    for name in decl:
        assert hasattr(lib, name), name


def test_unsupported_calls_return_minus_one_without_a_device(large_lib):
    """-1 before any HIP call: run in a process where no GPU is visible, with null pointers"""
    code = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
t = ctypes.c_double(0.0)
rc = [lib.smfft_large_launch(None, None, n, c, 0, None) for n, c in ((4096, 1), (32768, 1), (8192, -1), (16384, -5), (0, 1))]
rc += [lib.smfft_large_benchmark(None, None, n, c, 1, ctypes.byref(t)) for n, c in ((4096, 1), (8192, -1))]
rc += [lib.smfft_large_grid(4096), lib.smfft_large_grid(12288)]
print(rc, t.value)
sys.exit(0 if rc == [-1] * 9 and t.value == 0.0 else 1)
"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code, large_lib], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stdout + p.stderr


def test_import_does_not_load_the_large_library():
    code = "import sys; sys.path.insert(0, sys.argv[1]); import smfft_amd, smfft_amd.large as l; assert l._lib is None; print('ok')"
    p = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout + p.stderr


# ---- kernel inventory of libsmfft_large.so ---------------------------------------------------------------
def test_every_large_kernel_is_in_the_inventory_with_its_tests(large_lib):
    ac.check_inventory(large_lib, linv.KERNELS, "smfft_large_", 4)

"""The decimation-in-frequency transform (include/smfft/smfft_dif.hpp) on the CPU: its NumPy model (tools/dif_ladder_model.py) is
fft(x)[bitrev] and the no-reorder DIT transform inverts it, the header computes the model's indices and twiddles, the gfx950 code of
the DIF kernels keeps the library's budgets and the convolution chain needs fewer barriers than the natural-order one, and the C ABI
declares and exports the new entry points.  No GPU code is run (hipcc cross-compiles gfx950)."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle.np_reference import bitrev_indices, ct_c2c

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dif_ladder_model as dm  # noqa: E402
from inst_flags import part_flags  # noqa: E402
from quarter_swizzle import product_swizzle  # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fno-slp-vectorize", "-I" + os.path.join(ROOT, "include")]
SIZES = [32, 64, 128, 256, 512, 1024, 2048, 4096]
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("inverse", [0, 1])
def test_model_is_the_bit_reversed_dft(n, inverse):
    rng = np.random.default_rng(10 * n + inverse)
    for wave64 in ((False, True) if n <= 128 else (False,)):
        per_block = dm.block_threads(n, wave64) * 4 // n
        x = rng.standard_normal((3 * per_block, n)) + 1j * rng.standard_normal((3 * per_block, n))
        got = dm.transform(n, inverse, x, wave64=wave64)
        spec = np.fft.ifft(x, axis=-1) * n if inverse else np.fft.fft(x.astype(np.complex128), axis=-1)
        want = spec[..., bitrev_indices(n)]
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (n, inverse, wave64)
        # the no-reorder DIT transform of the other direction is its exact inverse partner
        back = ct_c2c(got, inverse=not inverse, reorder=False)
        assert np.max(np.abs(back - n * x)) <= 1e-12 * n * np.max(np.abs(x)), (n, inverse, wave64)


def test_model_counts_the_ladders_lds_traffic():
    """the register form: 4 (passes - 1) LDS accesses per thread each way, within 17 % of conflict free (what is left: the
    2-way stores of one pass, as in the DIT ladder); workgroup barriers only behind the cross-wave passes"""
    for n, barriers in ((256, 0), (512, 1), (1024, 1), (2048, 2), (4096, 2)):
        r, w, cycles, ideal, b = dm.lds_report(n)
        plan = dm.Plan(n)
        assert r == w == 4 * (plan.passes - 1), (n, r, w)
        assert cycles <= 1.17 * ideal, (n, cycles, ideal)
        assert b == barriers, (n, b)


# ------------------------------------------------------------------------------------------------ header == model
@needs_hipcc
def test_header_computes_the_models_indices_and_twiddles(tmp_path):
    src = tmp_path / "dif_plan.hip"
    src.write_text(r'''
#include <cstdio>
#include "smfft_device.hpp"
template <int N>
void dump() {
    using D = smfft::DifPlan<N>;
    constexpr smfft::QuarterTwiddleRows<N> rows{};
    printf("N %d %d\n", N, D::kPasses);
    for (int j = 0; j < D::kPasses; ++j)
        for (int t = 0; t < N / 4; ++t) {
            const int i = D::twiddle_index(j, t);
            const smfft::TwiddleValue w = i >= 0 ? rows.w[D::twiddle_row_entry(j, t)] : smfft::TwiddleValue{1.f, 0.f};
            printf("%d %d %d %d %d %d %d %a %a %d\n", j, t, D::element(j, t, 0), D::element(j, t, 1), D::element(j, t, 2), D::element(j, t, 3),
                   i, (double)w.x, (double)w.y, (int)D::crosses_waves(j));
        }
}
int main() {
    dump<32>(); dump<64>(); dump<128>(); dump<256>(); dump<512>(); dump<1024>(); dump<2048>(); dump<4096>();
    for (int i = 0; i < 4096; ++i) printf("S %d\n", smfft::quarter_swizzle(i));
    return 0;
}
''')
    exe = tmp_path / "dif_plan"
    subprocess.check_call([HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                          stderr=subprocess.DEVNULL)
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    seen, swz = 0, []
    plan = None
    for line in lines:
        f = line.split()
        if not f:
            continue
        if f[0] == "N":
            plan = dm.Plan(int(f[1]))
            assert int(f[2]) == plan.passes
            continue
        if f[0] == "S":
            swz.append(int(f[1]))
            continue
        j, t = int(f[0]), int(f[1])
        assert [int(v) for v in f[2:6]] == [plan.element(j, t, m) for m in range(4)], line
        assert int(f[6]) == plan.twiddle_index(j, t), line
        assert bool(int(f[9])) == plan.crosses_waves(j), line
        i = plan.twiddle_index(j, t)
        want = np.exp(-2j * np.pi * max(i, 0) / 4096)
        assert abs(float.fromhex(f[7]) - want.real) < 1e-7 and abs(float.fromhex(f[8]) - want.imag) < 1e-7, line
        seen += 1
    assert seen == sum(dm.Plan(n).passes * n // 4 for n in SIZES)
    assert swz == [product_swizzle(i) for i in range(4096)]


# ------------------------------------------------------------------------------------------------ gfx950 code
def _demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return [re.sub(r"\(.*", "", o).replace("void ", "") for o in out]


def _asm(rel, extra=()):
    out = f"/tmp/smfft_test_dif_{os.getpid()}_{abs(hash((rel,) + tuple(extra)))}.s"
    p = subprocess.run([HIPCC] + FLAGS + list(extra) + ["-S", "--cuda-device-only", os.path.join(ROOT, rel), "-o", out], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    text = open(out).read()
    os.remove(out)
    return text


def _resources(n):
    src = os.path.join(ROOT, "smfft_amd", "csrc", "smfft_inst.hip")
    p = subprocess.run([HIPCC] + FLAGS + part_flags(n, 1) + [f"-DSMFFT_N={n}", "-c", src, "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    rows, cur = [], None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = {"mangled": m.group(1)}
            rows.append(cur)
            continue
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    for r, name in zip(rows, _demangle([r["mangled"] for r in rows])):
        r["name"] = name
    return {r["name"]: r for r in rows}


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    with ThreadPoolExecutor(max_workers=4) as ex:
        dif = ex.submit(_asm, "examples/dif_convolution.hip")
        ref = ex.submit(_asm, "examples/reference_shape_kernel.hip")
        inst = {n: ex.submit(_asm, "smfft_amd/csrc/smfft_inst.hip", part_flags(n, 1) + [f"-DSMFFT_N={n}"]) for n in (32, 1024, 4096)}
        res = ex.submit(_resources, 1024)
        return {"dif": dif.result(), "ref": ref.result(), "inst": {n: f.result() for n, f in inst.items()}, "res": res.result()}


def _kernel(isa, frag):
    m = re.search(r"^(_Z\d+%s\w*):[^\n]*\n(.*?)\n\s*s_endpgm" % frag, isa, re.S | re.M)
    assert m, frag
    return m.group(1), [l.strip() for l in m.group(2).split("\n")]


def _no_scratch(isa, pattern):
    names = re.findall(r"^(_Z\w*(?:%s)\w*):" % pattern, isa, re.M)
    for mangled in names:
        _, body = _kernel(isa, re.escape(mangled[2:].lstrip("0123456789")))
        assert not [l for l in body if l.startswith("scratch_")], mangled
        d = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(mangled), isa, re.S)
        assert d, mangled
        seg = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", d.group(1))
        assert seg and int(seg.group(1)) == 0, (mangled, seg and seg.group(1))
    return len(names)


def test_dif_kernels_have_no_scratch_and_no_private_segment(built):
    assert _no_scratch(built["dif"], "user_dif_kernel|user_convolution_kernel_dif") == 2 * (8 + 3) + 2 * 5 + 5
    for n, isa in built["inst"].items():
        assert _no_scratch(isa, "SMFFT_DIF_external") == 2, n


def test_dif_external_kernel_budget(built):
    """SMFFT_DIF_external<FFT_1024_*_noreorder> within the limits of the headline kernel SMFFT_DIT_external<FFT_1024_forward>: no scratch, at
    least 3 waves per SIMD, at most 40 KiB of LDS"""
    res = built["res"]
    assert "SMFFT_DIT_external<FFT_1024_forward>" in res
    for name in ("SMFFT_DIF_external<FFT_1024_forward_noreorder>", "SMFFT_DIF_external<FFT_1024_inverse_noreorder>"):
        r = res[name]
        assert r["scratch"] == 0 and r["occ"] >= 3 and r["lds"] <= 40 * 1024, (name, r)


def test_dif_chain_has_fewer_barriers_than_the_natural_order_chain(built):
    """user_convolution_kernel_dif<FFT_1024_*_noreorder> (forward DIF -> .* Hb -> inverse DIT without reorder, registers throughout):
    strictly fewer workgroup barriers than user_convolution_kernel_registers<FFT_1024_forward, FFT_1024_inverse> -- no barrier between the two
    transforms, no reordering in either"""
    _, chain = _kernel(built["dif"], "user_convolution_kernel_difI26FFT_1024_forward_noreorder26FFT_1024_inverse_noreorderE")
    _, regs = _kernel(built["ref"], "user_convolution_kernel_registersI16FFT_1024_forward16FFT_1024_inverseE")
    nb = lambda body: sum(l.startswith("s_barrier") for l in body)  # noqa: E731
    assert 1 <= nb(chain) < nb(regs), (nb(chain), nb(regs))


def test_dif_chain_fetches_everything_before_its_second_barrier(built):
    """the rule test_convolution_example_fetches_its_filter_with_the_series applies to the natural-order chains: every global load (series,
    filter, both transforms' twiddles) in front of the kernel's second barrier"""
    for n in (1024, 4096):
        _, body = _kernel(built["dif"], f"user_convolution_kernel_difI{len(f'FFT_{n}_forward_noreorder')}FFT_{n}_forward_noreorder")
        barriers = [i for i, l in enumerate(body) if l.startswith("s_barrier")]
        loads = [i for i, l in enumerate(body) if l.startswith("global_load")]
        assert len(loads) >= 8 and len(barriers) >= 2, (n, len(loads), len(barriers))
        assert max(loads) < barriers[1], (n, max(loads), barriers[:3])


# ------------------------------------------------------------------------------------------------ C ABI
def test_dif_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "smfft.h")).read()
    for decl in ("int smfft_ct_dif_external_benchmark(const void* d_input, void* d_output, int FFT_size, int nFFTs, int inverse, double* FFT_time);",
                 "int smfft_ct_dif_launch(const void* d_input, void* d_output, int FFT_size, int nFFTs, int inverse, void* hip_stream);"):
        assert decl in header, decl
    import smfft_amd
    for name in ("smfft_ct_dif_external_benchmark", "smfft_ct_dif_launch"):
        assert name in smfft_amd.api.EXPORTED_C_SYMBOLS
        assert getattr(smfft_amd.lib, name)
    assert callable(smfft_amd.c2c_dif) and callable(smfft_amd.launch_dif)
    nm = subprocess.run(["nm", "-D", "--defined-only", smfft_amd.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T smfft_ct_dif_external_benchmark$", nm, re.M) and re.search(r" T smfft_ct_dif_launch$", nm, re.M)

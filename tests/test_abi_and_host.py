"""CPU-side checks (no GPU, no compute calls): the C-ABI library loads and exports every symbol
include/smfft.h declares plus the reference's own C++-linkage names; host-side logic."""
import ctypes
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def built(built_product):
    return built_product


def _reference_abi():
    """What the reference declares at the drop-in boundary (its parameter classes' values, the symbols its harnesses bind),
    stored with the tests: tests/golden/reference_abi.json."""
    return json.load(open(os.path.join(ROOT, "tests", "golden", "reference_abi.json")))


def _declared_c_functions():
    text = open(os.path.join(ROOT, "include", "smfft.h")).read() + open(os.path.join(ROOT, "include", "smfft_debug.h")).read()      # (the test-only entry points too)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(smfft_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported(built):
    lib = ctypes.CDLL(built)
    names = _declared_c_functions()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/smfft.h but not exported"


def test_python_mirror_matches_header(built):
    import smfft_amd.api as api
    assert sorted(api.EXPORTED_C_SYMBOLS) == _declared_c_functions()
    assert api.lib.smfft_version().startswith(b"smfft_amd")
    assert api.lib.smfft_get_nreuses() == 100 == api.NREUSES


def test_reference_cxx_symbols_are_exported(built):
    """The reference's FFT.c binds these by C++ linkage (CT/FFT.c:80-81, ST/FFT.c:79-81,
    RC/FFT.c:188-191 + the L2 functions of the .cu files)."""
    import smfft_amd.api as api
    out = subprocess.check_output(["nm", "-D", "--defined-only", built], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in api.EXPORTED_CXX_SYMBOLS:
        assert sym in exported, sym
    demangled = subprocess.check_output(["c++filt"] + list(api.EXPORTED_CXX_SYMBOLS), text=True).splitlines()
    assert "FFT_init()" in demangled
    assert any(d.startswith("FFT_external_benchmark(HIP_vector_type<float, 2u>*, HIP_vector_type<float, 2u>*, int, int, bool, bool, double*)") for d in demangled)
    assert any(d.startswith("GPU_smFFT_4elements(") for d in demangled)


def test_no_oracle_in_product(built):
    """The product library must not link or load anything from oracle/."""
    needed = subprocess.check_output(["readelf", "-d", built], text=True)
    assert "oracle" not in needed
    for root, _, files in os.walk(os.path.join(ROOT, "smfft_amd")):
        for f in files:
            if f.endswith((".py", ".hpp", ".hip", ".h")):
                src = open(os.path.join(root, f)).read()
                assert "liboracle" not in src and "from oracle" not in src and "import oracle" not in src, f


def test_missing_library_fails_loudly(tmp_path):
    code = "import os; os.environ['SMFFT_AMD_LIB']='/nonexistent/libsmfft_amd.so'; import smfft_amd"
    p = subprocess.run(["python", "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode != 0 and "no CPU fallback" in p.stderr


def test_parameter_classes_match_reference_names_and_values(tmp_path):
    """The 32 parameter classes carry the reference's names, and the members the reference defines keep the reference's
    VALUES (fft_exp, fft_length and its fractions, fft_direction, fft_reorder): a kernel written against them
    (README.md:48-60) sees what it saw upstream.  Checked by compiling the header with g++ and against the numbers of
    the reference's SM_FFT_parameters.cuh (stored in tests/golden/reference_abi.json).  Deliberate differences:
    warp = 64, fft_sm_required = 17 * fft_length / 16 (>= upstream's (fft_length / 32) * 33), and
    FFT_4096_inverse_noreorder::fft_direction = 1 (upstream 0, a typo)."""
    import shutil
    hdr_path = os.path.join(ROOT, "include", "smfft", "SM_FFT_parameters.hpp")
    hdr = open(hdr_path).read()
    names = [f"FFT_{n}_{suf}" for n in (32, 64, 128, 256, 512, 1024, 2048, 4096) for suf in ("forward", "forward_noreorder", "inverse", "inverse_noreorder")]
    for name in names:
        assert f"class {name} " in hdr
    members = ("fft_exp", "fft_sm_required", "fft_length", "fft_length_quarter", "fft_length_half", "fft_length_three_quarters", "fft_direction", "fft_reorder", "warp")
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = tmp_path / "params.cpp"
    body = "".join('printf("%s' % name + " %d" * len(members) + '\\n", ' + ", ".join(f"(int){name}::{m}" for m in members) + ");\n" for name in names)
    src.write_text('#include <cstdio>\n#include "smfft/SM_FFT_parameters.hpp"\nint main() {\n' + body + "return 0; }\n")
    exe = tmp_path / "params"
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        f = line.split()
        got[f[0]] = dict(zip(members, map(int, f[1:])))
    ref = _reference_abi()["parameter_classes"]
    assert set(names) <= set(ref)
    for name in names:
        n = int(name.split("_")[1])
        v = got[name]
        length = max(n, 128)
        want = {"fft_exp": n.bit_length() - 1, "fft_length": length, "fft_length_quarter": length // 4, "fft_length_half": length // 2,
                "fft_length_three_quarters": 3 * length // 4, "fft_direction": int("inverse" in name), "fft_reorder": int("noreorder" not in name)}
        for k, val in want.items():
            assert v[k] == val, (name, k)
            if not (name == "FFT_4096_inverse_noreorder" and k == "fft_direction"):
                assert ref[name][k] == val, (name, k, "reference value differs")
        assert v["warp"] == 64 and v["fft_sm_required"] == 17 * length // 16
        assert v["fft_sm_required"] >= ref[name]["fft_sm_required"]
    assert ref["FFT_4096_inverse_noreorder"]["fft_direction"] == 0   # the upstream typo this library does not reproduce
    # the wave64-full extension classes of the small lengths: one full 64-lane wave per block, everything else as their namesakes
    wave64 = [f"FFT_{n}_{suf}_wave64" for n in (32, 64, 128) for suf in ("forward", "forward_noreorder", "inverse", "inverse_noreorder")]
    for flags, block_of_upstream_names in (([], 128), (["-DSMFFT_WAVE64_SMALL=1"], 256)):
        body = "".join('printf("%s' % name + " %d" * len(members) + '\\n", ' + ", ".join(f"(int){name}::{m}" for m in members) + ");\n" for name in wave64 + names[:12])
        src.write_text('#include <cstdio>\n#include "smfft/SM_FFT_parameters.hpp"\nint main() {\n' + body + "return 0; }\n")
        subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)] + flags, check=True)
        for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
            f = line.split()
            v = dict(zip(members, map(int, f[1:])))
            n = int(f[0].split("_")[1])
            length = 256 if f[0].endswith("_wave64") else block_of_upstream_names
            assert v["fft_length"] == length and v["fft_length_quarter"] == length // 4 and v["fft_sm_required"] == 17 * length // 16, f[0]
            assert v["fft_exp"] == n.bit_length() - 1 and v["fft_direction"] == int("inverse" in f[0]) and v["fft_reorder"] == int("noreorder" not in f[0]), f[0]


def test_shard_range_tiles_batch():
    from smfft_amd.sharding import shard_range
    for nffts in (0, 1, 7, 8, 524288, 524289, 4194304 + 5):
        for world in (1, 2, 3, 4, 8):
            pos = 0
            for r in range(world):
                first, count = shard_range(nffts, r, world)
                assert first == pos and count in (nffts // world, nffts // world + 1)
                pos += count
            assert pos == nffts
    with pytest.raises(ValueError):
        shard_range(8, 2, 2)


def test_reference_style_harness_compiles_and_links_through_the_shim(built, tmp_path):
    """A translation unit written the way the reference's FFT.c is (CUDA header names, the reference's own prototypes
    with float2 and bool, C++ linkage, cudaDeviceReset) compiles with g++ against include/shim and links against
    libsmfft_amd.so + libsmfft_vendor.so: the drop-in boundary of INTEGRATION.md section A.  Link only: no GPU here."""
    import shutil
    import subprocess
    if shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("g++ / ROCm headers not available")
    root = os.path.join(os.path.dirname(__file__), "..")
    src = tmp_path / "main.c"
    src.write_text(
        "#include <cuda.h>\n#include <cuda_runtime.h>\n#include <cuda_runtime_api.h>\n#include <stdio.h>\n#include <stdlib.h>\n"
        "int GPU_smFFT_4elements(float2 *h_input, float2 *h_output, int FFT_size, int nFFTs, bool inverse, bool reorder, int nRuns, double *single_ex_time, double *multi_ex_time);\n"
        "int GPU_cuFFT(float2 *h_input, float2 *h_output, int FFT_size, int nFFTs, bool inverse, int nRuns, double *single_ex_time);\n"
        "int GPU_FFT_C2C_Stockham(float2 *h_input, float2 *h_smFFT_output, int FFT_size, int nFFTs, int nRuns, double *single_ex_time, double *multi_ex_time);\n"
        "int GPU_smFFT_R2C(float2 *h_output, float *h_input, int FFT_size, int nFFTs, int nRuns);\n"
        "int GPU_smFFT_C2R(float *h_output, float2 *h_input, int FFT_size, int nFFTs, int nRuns);\n"
        "int main(int argc, char **argv) {\n"
        "  if (argc < 99) return 0;   /* never runs the GPU part in this test */\n"
        "  float2 *a = (float2 *) malloc(1024*sizeof(float2)), *b = (float2 *) malloc(1024*sizeof(float2)); double t1, t2;\n"
        "  GPU_cuFFT(a, b, 1024, 1, false, 1, &t1);\n"
        "  GPU_smFFT_4elements(a, b, 1024, 1, false, true, 1, &t1, &t2);\n"
        "  GPU_FFT_C2C_Stockham(a, b, 1024, 1, 1, &t1, &t2);\n"
        "  GPU_smFFT_R2C(b, (float *) a, 1024, 1, 1); GPU_smFFT_C2R((float *) a, b, 1024, 1, 1);\n"
        "  cudaDeviceReset(); return 0; }\n")
    exe = tmp_path / "FFT.exe"
    cmd = ["g++", "-O1", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(root, "include", "shim"), "-I/opt/rocm/include", str(src), "-o", str(exe),
           "-L" + os.path.join(root, "smfft_amd"), "-lsmfft_amd", "-lsmfft_vendor", "-L/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath," + os.path.abspath(os.path.join(root, "smfft_amd")), "-Wl,-rpath,/opt/rocm/lib"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert subprocess.run([str(exe)], capture_output=True).returncode == 0   # argc < 99: exits before touching a device



@pytest.mark.parametrize("program", ["SMFFT_CooleyTukey_C2C", "SMFFT_Stockham_C2C", "SMFFT_Stockham_R2C_C2R"])
def test_the_references_own_harness_links_unchanged(built, tmp_path, program):
    """The reference's OWN host harness (its FFT.c, unedited) links against libsmfft_amd.so + libsmfft_vendor.so: every
    symbol it binds (GPU_smFFT_4elements, GPU_cuFFT, GPU_FFT_C2C_Stockham, GPU_smFFT_R2C/C2R, GPU_cuFFT_R2C/C2R, with
    the reference's C++ mangling, and hipDeviceReset through include/shim) is exported.  The symbols are the undefined
    ones of that FFT.c compiled with g++ against include/shim, stored in tests/golden/reference_abi.json; a translation
    unit that takes the address of each one under its exact mangled name is linked the way the harness is, and run
    with immediate binding so that the dynamic loader resolves every one.  Link only; the artefact lives in tmp_path."""
    import shutil
    if shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("g++ / ROCm headers not available")
    symbols = _reference_abi()["harness_symbols"][program]
    assert any("GPU_" in s for s in symbols) and "hipDeviceReset" in symbols
    src = tmp_path / "FFT.c"
    decls = "".join(f'extern "C" void ref_sym_{i}() __asm__("{s}");\n' for i, s in enumerate(symbols))
    refs = ", ".join(f"(void *) &ref_sym_{i}" for i in range(len(symbols)))
    src.write_text(decls + "#include <stdio.h>\nint main() {\n  void *bound[] = {" + refs + "};\n"
                   "  for (unsigned i = 0; i < sizeof(bound) / sizeof(bound[0]); ++i) if (!bound[i]) return 1;\n"
                   '  puts("FFT harness symbols bound"); return 0; }\n')
    exe = tmp_path / "FFT.exe"
    cmd = ["g++", "-O1", "-w", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include", "shim"), "-I/opt/rocm/include",
           str(src), "-o", str(exe), "-Wl,-z,now", "-Wl,--no-as-needed",
           "-L" + os.path.join(ROOT, "smfft_amd"), "-lsmfft_amd", "-lsmfft_vendor", "-L/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath," + os.path.join(ROOT, "smfft_amd"), "-Wl,-rpath,/opt/rocm/lib"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    # nothing is called: the addresses are only taken, so no device is touched
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, env=dict(os.environ, LD_BIND_NOW="1"))
    assert run.returncode == 0 and "FFT" in run.stdout, (run.returncode, run.stdout, run.stderr)
    exported = set()
    for lib in ("libsmfft_amd.so", "libsmfft_vendor.so"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "smfft_amd", lib)], text=True)
        exported |= {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in symbols:
        assert s == "hipDeviceReset" or s in exported, s

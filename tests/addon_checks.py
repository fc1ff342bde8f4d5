"""What the CPU tests of the add-on libraries share (test_large_cpu.py, test_large_real_cpu.py, test_large_fir_cpu.py, test_pfb_cpu.py,
test_pfb_real_cpu.py):
the per-length flags of the Makefile, the compile of a per-length object to gfx950 assembly as the Makefile compiles it, the fields of
a kernel descriptor, the declarations of a C header as ctypes signatures, and the walk through a kernel inventory."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "smfft_amd", "csrc")
# the Makefile's HIPFLAGS less -fPIC / -Wall, which change no device code; "-I" + CSRC is the -I. of the objects that have it
FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fno-slp-vectorize", "-I" + os.path.join(ROOT, "include")]
CTYPES = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "int": ctypes.c_int, "long long": ctypes.c_longlong,
          "double*": ctypes.POINTER(ctypes.c_double)}


def makefile_flags(prefix, n):
    """the words of the Makefile's line `<prefix>_FLAGS_<n> :=`"""
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(rf"{prefix}_FLAGS_{n}\s*:=(.*)", line)
        if m:
            return m.group(1).split()
    raise AssertionError(f"{prefix}_FLAGS_{n} missing from the Makefile")


def device_asm(src, extra, out):
    """the gfx950 assembly of src under FLAGS + extra, written to the path `out`"""
    p = subprocess.run([HIPCC] + FLAGS + extra + ["-S", "--cuda-device-only", str(src), "-o", str(out)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    with open(out) as f:
        return f.read()


def descriptors(asm):
    """{kernel name: the text of its .amdhsa_kernel block}, in the order of the file"""
    return dict(re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, flags=re.S))


def descriptor_field(descs, name, field):
    """the integer .amdhsa_<field> of kernel `name` in descs = descriptors(asm)"""
    assert name in descs, name
    m = re.search(rf"\.amdhsa_{field} (\d+)", descs[name])
    assert m, (name, field)
    return int(m.group(1))


def declarations(header):
    """{function: (result type, argument list)} of the smfft_* functions that include/<header> declares, as written there"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return {name: (res, args) for res, name, args in re.findall(r"\b(int|long long)\s+(smfft_\w+)\s*\(([^)]*)\)", text)}


def signature(res, args):
    """(restype, argtypes) of a declaration, in the form of the mirrors' SIGS"""
    return CTYPES[res], [CTYPES[re.sub(r"\s*\w+$", "", a.strip())] for a in args.split(",")]


INVENTORY_KINDS = ("tests", "bounds", "probes", "host")


def check_inventory(lib_path, kernels, call_prefix, count, kinds=INVENTORY_KINDS):
    """the library ships exactly the `count` kernels of the inventory `kernels`, and every entry names its C entry point and, per kind
    of `kinds`, tests that exist: GPU tests, except "host", the run of the kernel on the host (tests/hostsim), which needs no GPU.  An
    inventory whose kernels hostsim cannot run passes kinds without "host" and says why in its docstring."""
    from tests import test_kernel_inventory as kinv
    handles, stubs = kinv._shipped_kernels(lib_path)
    assert handles == stubs and len(handles) == count, (sorted(handles), sorted(stubs))
    assert handles == set(kernels), (sorted(handles ^ set(kernels)))
    assert set(kinds) <= set(INVENTORY_KINDS) and {"tests", "bounds", "probes"} <= set(kinds), kinds
    for name, entry in kernels.items():
        assert set(entry) == {"call"} | set(kinds), name
        assert entry["call"].startswith(call_prefix), name
        for key in kinds:
            assert entry[key], (name, key)
            for tid in entry[key]:
                m = re.fullmatch(r"(tests/test_\w+\.py)::(test_\w+)", tid)
                assert m, tid
                names, gpu = kinv._gpu_tests(os.path.join(ROOT, m.group(1)))
                assert m.group(2) in names and gpu == (key != "host"), tid

"""Every kernel libsmfft_amd.so ships is in tests/kernel_inventory.py with a GPU test that compares it with fp64 and one that runs
it on guarded buffers and one that probes it per element and in isolation (or a reason why it is not a transform), and every test the inventory names exists.  CPU only: the kernels are
enumerated from the built library's host-side kernel handles -- one data symbol per __global__ instantiation, whose demangled name is
the kernel's -- so nothing is recompiled."""
import ast
import os
import re
import shutil
import subprocess

import pytest

from tests import kernel_inventory as inv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nm():
    for tool in (shutil.which("nm"), "/opt/rocm/llvm/bin/llvm-nm"):
        if tool and os.path.exists(tool):
            return tool
    pytest.skip("no nm / llvm-nm to read the library's symbols")


def _strip_params(demangled):
    """'void ns::(anonymous namespace)::k<256>(float2 const*, ...)' -> 'ns::(anonymous namespace)::k<256>'"""
    name = demangled[len("void "):].replace("(anonymous namespace)", "\0")
    return name.split("(", 1)[0].replace("\0", "(anonymous namespace)")


def _shipped_kernels(lib):
    out = subprocess.run([_nm(), "-C", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    handles, stubs = set(), set()
    for line in out.splitlines():
        parts = line.split(" ", 2)
        if len(parts) != 3:
            continue
        kind, name = parts[1], parts[2]
        if not name.startswith("void "):
            continue
        if kind in "dDbBvVuRr":                           # the kernel handle: a data object named like the kernel
            handles.add(_strip_params(name))
        elif "__device_stub__" in name:                   # the host stub hipcc emits for every kernel (a function)
            stubs.add(_strip_params(name).replace("__device_stub__", ""))
    return handles, stubs


@pytest.fixture(scope="module")
def shipped(built_product):
    handles, stubs = _shipped_kernels(built_product)
    # the two ways of finding the kernels agree: every kernel has its stub, and no handle is some other data object
    assert handles == stubs, (sorted(handles - stubs), sorted(stubs - handles))
    return handles


def test_every_shipped_kernel_is_in_the_inventory(shipped):
    listed = set(inv.KERNELS) | set(inv.NOT_TRANSFORMS)
    assert not set(inv.KERNELS) & set(inv.NOT_TRANSFORMS)
    missing, stale = sorted(shipped - listed), sorted(listed - shipped)
    assert not missing, f"kernels the library ships without an inventory entry (tests/kernel_inventory.py): {missing}"
    assert not stale, f"inventory entries for kernels the library does not ship: {stale}"
    assert len(shipped) >= 100      # (the enumeration found the kernels at all)


def test_every_transform_names_a_call_and_an_fp64_test():
    for name, entry in inv.KERNELS.items():
        assert set(entry) == {"call", "tests", "bounds", "probes"}, name
        assert entry["call"].startswith("smfft_"), name
        assert entry["tests"], f"{name}: no GPU test compares it with fp64"
        assert entry["bounds"], f"{name}: no GPU test runs it on guarded buffers (tests/test_buffers_gpu.py)"
        assert entry["probes"], f"{name}: no GPU test probes it per element and in isolation (tests/test_probes_gpu.py)"
    for name, reason in inv.NOT_TRANSFORMS.items():
        assert reason.strip(), name


def _gpu_tests(path):
    """names of the module-level test functions of a test file, and whether the module is marked gpu"""
    tree = ast.parse(open(path).read(), path)
    names = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    gpu = any(isinstance(n, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "pytestmark" for t in n.targets)
              and "gpu" in ast.unparse(n.value) for n in tree.body)
    return names, gpu


def _named_tests_exist_and_are_gpu_tests(key):
    files = {}
    for name, entry in inv.KERNELS.items():
        for tid in entry[key]:
            m = re.fullmatch(r"(tests/test_\w+\.py)::(test_\w+)", tid)
            assert m, f"{name}: malformed test id {tid!r}"
            path = os.path.join(ROOT, m.group(1))
            assert os.path.exists(path), f"{name}: {m.group(1)} does not exist"
            if path not in files:
                files[path] = _gpu_tests(path)
            names, gpu = files[path]
            assert m.group(2) in names, f"{name}: {tid} does not exist"
            assert gpu, f"{name}: {m.group(1)} is not a GPU test module"


def test_named_tests_exist_and_are_gpu_tests():
    _named_tests_exist_and_are_gpu_tests("tests")


def test_bounds_tests_exist_and_are_gpu_tests():
    _named_tests_exist_and_are_gpu_tests("bounds")


def test_probes_tests_exist_and_are_gpu_tests():
    _named_tests_exist_and_are_gpu_tests("probes")

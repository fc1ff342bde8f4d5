"""Every public function of the header-only device API is in tests/device_function_inventory.py with GPU tests that compare it with
fp64 and GPU tests that probe it per element and in isolation (run by some case of tests/probe_cases.py HEADER_CASES), and every
test the inventory names exists and is a GPU test.  CPU only: the functions are read from the header text."""
import os
import re

from tests import device_function_inventory as inv
from tests import probe_cases as pc
from tests.test_kernel_inventory import _gpu_tests

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ["include/smfft/smfft_device_functions.hpp", "include/smfft/smfft_dif.hpp"]
PUBLIC_NAMESPACES = {(), ("smfft", "tiled")}

_DECL = re.compile(r"template\s*<[^;{]*?>\s*(?:__device__|__global__)\s+void\s+(\w+)\s*\(")
_TOKEN = re.compile(r"namespace\s+(\w+)\s*\{|\{|\}")


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def public_functions(text):
    """qualified names of the `template <...> __device__ / __global__ void NAME(` declarations at global scope or in namespace
    smfft::tiled (anything declared inside a function or class body, or in another namespace, is not API)"""
    text = _strip_comments(text)
    events = sorted([(m.start(), "decl", m.group(1)) for m in _DECL.finditer(text)] +
                    [(m.start(), "tok", m.group(0), m.group(1)) for m in _TOKEN.finditer(text)], key=lambda e: e[0])
    stack, found = [], set()
    for ev in events:
        if ev[1] == "decl":
            if all(kind == "ns" for kind, _ in stack):
                path = tuple(name for _, name in stack)
                if path in PUBLIC_NAMESPACES:
                    found.add("::".join(path + (ev[2],)))
        elif ev[3]:
            stack.append(("ns", ev[3]))
        elif ev[2] == "{":
            stack.append(("block", None))
        else:
            assert stack, "unbalanced braces"
            stack.pop()
    assert not stack, "unbalanced braces"
    return found


def _header_functions():
    found = set()
    for h in HEADERS:
        found |= public_functions(open(os.path.join(ROOT, h)).read())
    return found


def test_the_parser_sees_what_it_should():
    text = """
    namespace smfft { template <int N> __device__ __forceinline__ void helper(float2* s) { }
    namespace tiled { template <class P> __device__ void tiled_fn(float2* s) { if (1) { } } }  // namespace tiled
    }  // namespace smfft
    // template <class P> __device__ void commented_out(float2* s);
    template <class P> __device__ void contract_fn(float2* s) { }
    template <class P, class D>
    __global__ void kernel(float2* a, float2* b) { }
    """
    assert public_functions(text) == {"smfft::tiled::tiled_fn", "contract_fn", "kernel"}


def test_every_public_device_function_is_in_the_inventory():
    found = _header_functions()
    missing, stale = sorted(found - set(inv.FUNCTIONS)), sorted(set(inv.FUNCTIONS) - found)
    assert not missing, f"public device functions without an inventory entry (tests/device_function_inventory.py): {missing}"
    assert not stale, f"inventory entries for functions the headers do not declare: {stale}"
    assert len(found) >= 20      # (the parser found the functions at all)


def test_every_entry_names_classes_and_fp64_tests():
    for name, entry in inv.FUNCTIONS.items():
        assert set(entry) == {"classes", "tests", "probes"}, name
        assert entry["classes"].strip(), name
        assert entry["tests"], f"{name}: no GPU test compares it with fp64"
        assert entry["probes"], f"{name}: no GPU test probes it per element and in isolation (tests/test_device_probes_gpu.py)"


def test_every_function_has_probe_cases():
    """each function is run by a case of HEADER_CASES (through an entry point of probe_cases.HEADER_FUNCS that names it), and every
    name there is an inventory function"""
    run = {}
    for c in pc.HEADER_CASES:
        for name in pc.HEADER_FUNCS[c.func][1]:
            run.setdefault(name, set()).add(c.id)
    assert set(run) <= set(inv.FUNCTIONS), sorted(set(run) - set(inv.FUNCTIONS))
    missing = sorted(set(inv.FUNCTIONS) - set(run))
    assert not missing, f"inventory functions that no probe case runs: {missing}"


def _named_tests_exist_and_are_gpu_tests(key):
    files = {}
    for name, entry in inv.FUNCTIONS.items():
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


def test_probes_tests_exist_and_are_gpu_tests():
    _named_tests_exist_and_are_gpu_tests("probes")

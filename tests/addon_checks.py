"""What the CPU tests of the add-on libraries share (test_large_cpu.py, test_large_real_cpu.py, test_large_fir_cpu.py, test_pfb_cpu.py,
test_pfb_real_cpu.py, test_fir_real_cpu.py, the eight test_sm_*_cpu.py of the row libraries; the FIR checks at the end serve
test_fir_cpu.py, the main library's bank, too): the per-length flags of the Makefile, the compile of a per-length object -- or of all
of a library's -- to gfx950 assembly as the Makefile compiles it, the fields of a kernel descriptor, the occupancy a register count
allows, the declarations of a C header as ctypes signatures, the exported symbols, the walk through a kernel inventory, and what every
mirror's import and the no-device subprocesses are held to."""
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


def occupancy(vgprs):
    """waves per SIMD that the vector registers allow: 512 registers in granules of 8"""
    return 512 // (-(-vgprs // 8) * 8)


def addon_isa(stem, prefix, sizes, tmp, extra=()):
    """{N: gfx950 assembly of <stem>_<N>.o as the Makefile compiles it: -I. and <prefix>_FLAGS_<N>, then `extra`}"""
    import concurrent.futures

    def compile_one(n):
        flags = ["-I" + CSRC] + makefile_flags(prefix, n) + [f"-DSMFFT_{prefix}_N={n}"] + list(extra)
        return device_asm(os.path.join(CSRC, stem + ".hip"), flags, tmp / f"{stem}_{n}.s")
    with concurrent.futures.ThreadPoolExecutor(len(sizes)) as pool:
        return dict(zip(sizes, pool.map(compile_one, sizes)))


def check_exports(lib_path, names):
    """the library's defined dynamic symbols named smfft_* are exactly `names`"""
    nm = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r" T (smfft_\w+)$", nm, re.M)) == sorted(names)


def check_isa_identity_lists(stem, prefix, sizes):
    """tools/isa_identity.py compiles the library's per-length objects with the Makefile's flags and -I., like the other add-ons' (the
    tool itself needs the history of a git checkout and minutes of compiling: it is run by hand)"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_identity
    assert (stem, prefix, sizes, True) in isa_identity.ADDONS
    names = [u[0] for u in isa_identity.units(ROOT)]
    assert all(f"{stem}_{n}" in names for n in sizes) and len(names) == len(set(names))


def check_import_does_not_load(module, lib_stem):
    """importing smfft_amd.<module> maps no lib<lib_stem>: the mirror loads its library on first use"""
    import sys
    code = (f"import sys; sys.path.insert(0, sys.argv[1]); import smfft_amd, smfft_amd.{module} as l; assert l._lib is None; "
            f"maps = open('/proc/self/maps').read(); assert 'lib{lib_stem}' not in maps; print('ok')")
    p = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout + p.stderr


# pasted in front of the scripts of the no-device subprocesses: f(*a, **k) raises exc, or the script ends with a message
REFUSED = '''
def refused(exc, f, *a, **k):
    try:
        f(*a, **k)
    except exc:
        return
    raise SystemExit(f"{f.__name__}{a}{k} was not refused with {exc.__name__}")
'''


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


# ------------------------------------------------------------------------------------------------ the two polyphase filter banks
# What test_pfb_cpu.py and test_pfb_real_cpu.py hold both banks to.  A bank is named by its source stem ("smfft_pfb"), which is also the
# prefix of its C functions, its Makefile prefix ("PFB") and its kernel ("pfb_kernel").
PFB_SIZES = (256, 512, 1024, 2048, 4096)
PFB_KERNEL_HEADER = os.path.join(CSRC, "smfft_pfb_kernel.hpp")      # the one kernel body and its kWorkgroupsPerCu
PFB_WORKGROUPS_PER_CU = 3
PFB_VGPR_BUDGET = 168          # three waves per SIMD: 512 registers / 3, in granules of 8; the persistent grid rests on it
LDS_PER_CU = 160 * 1024


def pfb_kernels(text, kernel):
    """{mangled name: the stripped lines of its body} of the instantiations of `kernel` in an assembly text"""
    found = {}
    for m in re.finditer(r"^(_Z\w*%s\w*):[^\n]*\n(.*?)\n\s*s_endpgm" % kernel, text, re.S | re.M):
        found[m.group(1)] = [line.strip() for line in m.group(2).split("\n")]
    return found


def check_pfb_kernel_rules(isa, kernel):
    """two kernels per length and nothing else, ten in all: no scratch, no v_sin / v_cos, no packed f32, the LDS of 4096 points and the
    VGPRs of three workgroups per compute unit, the figure the shared kernel header launches the persistent grid with"""
    assert re.search(r"constexpr int kWorkgroupsPerCu = %d;" % PFB_WORKGROUPS_PER_CU, open(PFB_KERNEL_HEADER).read())
    total = 0
    for n, text in isa.items():
        kernels, descs = pfb_kernels(text, kernel), descriptors(text)
        assert len(kernels) == 2 and len(descs) == 2, (n, sorted(kernels), sorted(descs))          # complex and power, nothing else
        total += len(kernels)
        for name, body in kernels.items():
            assert "%sILi%dE" % (kernel, n) in name
            assert not [line for line in body if line.startswith("scratch_")], name
            assert not [line for line in body if re.match(r"v_(sin|cos)_", line)], name
            assert not [line for line in body if re.match(r"v_pk_\w+_f32", line)], name
            assert descriptor_field(descs, name, "private_segment_fixed_size") == 0, name
            vgprs, lds = descriptor_field(descs, name, "next_free_vgpr"), descriptor_field(descs, name, "group_segment_fixed_size")
            print(f"N={n:5d} {'power  ' if 'ELi1EEE' in name else 'complex'}: {vgprs} VGPRs, {lds} B of LDS")
            assert lds == 4096 // 16 * 17 * 8 and PFB_WORKGROUPS_PER_CU * lds <= LDS_PER_CU, name
            assert vgprs <= PFB_VGPR_BUDGET, (name, vgprs)
    assert total == 10


def check_pfb_signal_loads(isa, kernel, signal, tap, arithmetic):
    """the sixteen signal loads of one tap (lines matching `signal`; the kernel's only non-temporal loads) are contiguous in the
    instruction stream up to address arithmetic (lines matching `arithmetic`), with no branch, barrier or vmcnt(0) between the first and
    the last, and sit in a loop (a backward branch follows them); its sixteen coefficient loads (lines matching `tap`) follow them
    inside the loop"""
    for n, text in isa.items():
        for name, body in pfb_kernels(text, kernel).items():
            loads = [i for i, line in enumerate(body) if re.match(signal, line)]
            assert len(loads) == 16, (name, len(loads))
            assert len([line for line in body if line.startswith("global_load") and line.endswith(" nt")]) == 16, name
            between = body[loads[0]:loads[-1] + 1]
            assert not [line for line in between if line.startswith(("s_cbranch", "s_branch", "s_setpc", "s_barrier"))], name
            assert not [line for line in between if re.search(r"vmcnt\(0\)", line)], name
            others = [line for line in between if line and not line.startswith("global_load_dwordx2")]
            assert all(re.match(arithmetic, line) for line in others), (name, others)
            # the loop: the first label before the loads is the target of the first branch after them
            label = next(line for line in reversed(body[:loads[0]]) if re.match(r"\.LBB\d+_\d+:", line)).split(":")[0]
            branch = next(line for line in body[loads[-1]:] if line.startswith("s_cbranch"))
            assert branch.split()[-1] == label, (name, label, branch)
            end = body.index(branch, loads[-1])
            taps = [i for i in range(loads[-1] + 1, end) if re.match(tap, body[i])]
            assert len(taps) == 16, (name, len(taps))


def pfb_names(stem):
    return tuple(f"{stem}_{f}" for f in ("frames", "launch", "benchmark", "launch_tuned", "default_tile_run"))


def check_pfb_declarations(mirror, stem, phrases):
    """include/<stem>.h says what is out of scope (`phrases`) and declares exactly the five functions of the mirror's SIGS"""
    header = open(os.path.join(ROOT, "include", stem + ".h")).read()
    for phrase in phrases:
        assert phrase in header, phrase
    decl = declarations(stem + ".h")
    assert sorted(decl) == sorted(mirror.SIGS) == sorted(pfb_names(stem))
    for name, (res, args) in decl.items():
        assert mirror.SIGS[name] == signature(res, args), name
    # launch_tuned = the arguments of launch + tile_run; benchmark = launch with the timer in the stream's place
    assert mirror.SIGS[stem + "_launch_tuned"][1] == mirror.SIGS[stem + "_launch"][1] + [ctypes.c_int]
    assert mirror.SIGS[stem + "_benchmark"][1][:-1] == mirror.SIGS[stem + "_launch"][1][:-1]
    assert mirror.SIZES == PFB_SIZES


def check_pfb_exports(mirror, stem):
    nm = subprocess.run(["nm", "-D", "--defined-only", mirror.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r" T (smfft_\w+)$", nm, re.M)) == sorted(pfb_names(stem))


def check_pfb_rejections(mirror, stem, samples, bad_lengths):
    """all validation happens before any HIP call: these return -1 (or 0 when there is no whole frame) with no device and null pointers.
    samples: of the signal per channel of a frame (1 complex, 2 real); bad_lengths: (L, C, N, P) with a signal length the bank refuses
    at a supported shape"""
    lib = mirror.lib()
    frames, launch, benchmark, launch_tuned, default_tile_run = (getattr(lib, name) for name in pfb_names(stem))
    t = ctypes.c_double(0.0)
    bad = [(1 << 20, 1, n, 4) for n in (0, 128, 1000, 8192, -1024)] + [(1 << 20, 1, 1024, p) for p in (0, 33, -1)]
    bad += [(1 << 20, c, 1024, 4) for c in (0, -1)] + list(bad_lengths)
    for L, C, N, P in bad:
        for power in (0, 1):
            assert launch(None, L, C, None, N, P, power, None, None) == -1, (L, C, N, P)
            assert launch_tuned(None, L, C, None, N, P, power, None, None, 3) == -1, (L, C, N, P)
            assert benchmark(None, L, C, None, N, P, power, None, ctypes.byref(t)) == -1, (L, C, N, P)
    assert launch_tuned(None, 1 << 20, 1, None, 1024, 4, 0, None, None, -1) == -1
    # no whole frame is not an error: nothing is launched
    for L in (0, samples * 1023, samples * (4 * 1024 - 1)):
        for power in (0, 1):
            assert launch(None, L, 2, None, 1024, 4, power, None, None) == 0
            assert launch_tuned(None, L, 2, None, 1024, 4, power, None, None, 7) == 0
            assert benchmark(None, L, 2, None, 1024, 4, power, None, ctypes.byref(t)) == 0
    assert t.value == 0.0
    for n in (0, 128, 1000, 8192):
        assert frames(1 << 20, n, 4) == -1 and default_tile_run(n, 4) == -1
    for p in (0, 33, -1):
        assert frames(1 << 20, 1024, p) == -1 and default_tile_run(1024, p) == -1
    for L, _, N, P in bad_lengths:
        assert frames(L, N, P) == -1, (L, N, P)


# ------------------------------------------------------------------------------------------------ the three FIR filter banks
# What test_fir_cpu.py, test_fir_real_cpu.py and test_large_fir_cpu.py hold their banks to.  A bank is named by the prefix of its C
# functions ("smfft_fir_real") and the lengths it serves.
def fir_taps_cases(n):
    return sorted({1, 2, 17, n // 4 + 1, n // 2, n - 1})


def fir_length_cases(n, m):
    """L < M, L < V, L = V, L = k V and L = k V +- 1; a pair and a lone segment, a second segment three outputs short, and
    (2F + 1) V - 3: more than one workgroup tile of pairs with a ragged last segment"""
    v, f = n - m + 1, max(1, 4096 // n)
    return sorted({1, max(1, m // 2), max(1, v // 3), v, v + 1, 2 * v, 2 * v + 1, 3 * v - 1, 3 * v, 3 * v + 1, (2 * f + 1) * v - 3}
                  | ({2 * v - 3} if v > 2 else set()))


def fir_names(prefix):
    return tuple(f"{prefix}_{f}" for f in ("prepare", "launch", "benchmark"))


def check_fir_rejections(lib_path, prefix, sizes):
    """-1 (or 0 for an empty signal) before any HIP call: run in a process where no GPU is visible, with null pointers.  Every length
    next to the bank's, every tap count outside 1 ... N - 1, and counts and lengths that are not positive"""
    import sys
    code = r"""
import ctypes, sys
lib, prefix, sizes = ctypes.CDLL(sys.argv[1]), sys.argv[2], [int(a) for a in sys.argv[3:]]
prepare, launch, benchmark = (getattr(lib, prefix + "_" + f) for f in ("prepare", "launch", "benchmark"))
ll = ctypes.c_longlong
t = ctypes.c_double(0.0)
lo, hi = sizes[0], sizes[-1]
off = [lo // 2, 2 * hi, lo - 1, 1000, 0, -lo]
bad = [(1000, 1, 1, 17, n) for n in off]                                                   # (L, C, K, M, N)
bad += [(1000, 1, 1, m, n) for n in sizes for m in (0, n, -3)]
bad += [(1000, 1, k, 17, n) for n in (lo, hi) for k in (0, -2)] + [(1000, c, 1, 17, n) for n in (lo, hi) for c in (0, -1)]
bad += [(L, 1, 1, 17, n) for n in (lo, hi) for L in (-1, -5)]
rc = []
for L, C, K, M, N in bad:
    for corr in (0, 1):
        rc.append(launch(None, ll(L), C, None, K, M, N, corr, None, None))
        rc.append(benchmark(None, ll(L), C, None, K, M, N, corr, None, ctypes.byref(t)))
for M, K, N in [(17, 1, n) for n in off] + [(m, 1, n) for n in sizes for m in (0, n)] + [(17, k, n) for n in (lo, hi) for k in (0, -1)]:
    rc.append(prepare(None, M, K, N, 0, None, None))
empty = [launch(None, ll(0), 1, None, 1, 17, n, 0, None, None) for n in sizes]
empty += [benchmark(None, ll(0), 1, None, 1, 17, n, 1, None, ctypes.byref(t)) for n in sizes]
print(rc, empty, t.value)
sys.exit(0 if rc == [-1] * len(rc) and empty == [0] * (2 * len(sizes)) and t.value == 0.0 else 1)
"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code, lib_path, prefix] + [str(n) for n in sizes], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stdout + p.stderr


def check_fir_wrappers_refuse(prepare, launch, sizes):
    """the mirror's prepare and launch turn the library's -1 into a RuntimeError and refuse an unknown mode themselves, before a device"""
    import pytest
    for n in (sizes[0], sizes[-1]):
        with pytest.raises(RuntimeError):
            launch(None, 1000, 1, None, 1, n, n, None)
        with pytest.raises(RuntimeError):
            prepare(None, None, 0, 1, n)
        with pytest.raises(ValueError):
            launch(None, 1000, 1, None, 1, 17, n, None, mode="xcorr")

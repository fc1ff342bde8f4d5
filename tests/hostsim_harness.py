"""What the host-run test modules (tests/test_large_hostsim.py, test_large_fir_hostsim.py, test_large_pfb_hostsim.py) share: the build of a
host library from tests/hostsim, the executor's schedules, guarded buffers, bit comparison and the barrier knock-out loop.  A plain
module: no tests, no fixtures."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "hostsim")
GUARD = 4096
GUARD_WORD = 0x7FC5A5A5    # a NaN of the guards' own, not the LDS prefill
OUT_WORD = 0xFFFFFFFF      # the NaN an output is prefilled with

ASC, DESC, WAVES, RANDOM = 0, 1, 2, 3
SEEDS = (1, 2, 3, 4)
# (schedule, seed, workgroups in descending order)
SCHEDULES = [(s, seed, d) for d in (0, 1) for s, seeds in ((ASC, (0,)), (DESC, (0,)), (WAVES, SEEDS), (RANDOM, SEEDS)) for seed in seeds]


# ---- the host library ---------------------------------------------------------------------------------------------------------------
def _compiler():
    for c in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    return None


def _cpu_has_fma():
    try:
        return any(" fma " in line + " " for line in open("/proc/cpuinfo") if line.startswith("flags"))
    except OSError:
        return False


def fma_flags():
    """the build that contracts, as the device does"""
    return ["-ffp-contract=fast"] + (["-mfma"] if _cpu_has_fma() else [])


_objects = {}      # (source, flags) -> a compile already started by this process, and its object file


def build(sources, lib_name, outdir, fp_flags, csrc_includes=False):
    """Compiles `sources` of tests/hostsim in parallel and links them with hostsim.cpp (last: its guard closes the LDS section) into
    outdir/lib_name, a directory of pytest's.  An object this process has built from the same source with the same flags is used again.
    -> the library's path"""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no clang++ that can build the host stub (address_space / ext_vector_type need clang)")
    os.makedirs(outdir, exist_ok=True)
    flags = ["-std=c++17", "-O2", "-fPIC", "-I" + HOSTSIM, "-I" + os.path.join(ROOT, "include")] + list(fp_flags)
    jobs = []
    for src in list(sources) + ["hostsim.cpp"]:
        own = flags + (["-I" + os.path.join(ROOT, "smfft_amd", "csrc")] if csrc_includes and src != "hostsim.cpp" else [])
        if (src, tuple(own)) not in _objects:
            obj = os.path.join(outdir, src.replace(".cpp", ".o"))
            _objects[src, tuple(own)] = subprocess.Popen([cxx] + own + ["-c", os.path.join(HOSTSIM, src), "-o", obj], stderr=subprocess.PIPE, text=True), obj
        jobs.append(_objects[src, tuple(own)])
    for proc, _ in jobs:
        err = proc.communicate()[1] if proc.returncode is None else ""
        assert proc.returncode == 0, err[-3000:]
    lib = os.path.join(outdir, lib_name)
    subprocess.check_call([cxx, "-shared", "-o", lib] + [obj for _, obj in jobs])
    return lib


# ---- data ---------------------------------------------------------------------------------------------------------------------------
def rand_complex(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def guarded(a, fill=None):
    """GUARD bytes, 8 more, the data, GUARD bytes; everything the guards' NaN pattern but the data: the bits of the array `a`, or the
    word `fill` in their place.  `a` may be a byte count: then the data is left as the guards are.  -> (words, byte offset of the data)"""
    nbytes = a if isinstance(a, int) else a.nbytes
    words = np.full((2 * GUARD + 8 + nbytes) // 4, GUARD_WORD, dtype=np.uint32)
    if not isinstance(a, int):
        words[(GUARD + 8) // 4:(GUARD + 8 + nbytes) // 4] = bits(a) if fill is None else fill
    return words, GUARD + 8


def payload(words, off, shape, dtype=np.complex64):
    """a copy of the data of a guarded buffer"""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize // 4
    return words[off // 4:off // 4 + n].view(dtype).reshape(shape).copy()


# ---- barrier knock-out ------------------------------------------------------------------------------------------------------------------
def knock_out(table, run_base, run_without, label):
    """table: one entry per barrier of a period, `needed` or `redundant: reason`.  run_base() -> (output, barriers per workgroup) of the
    shipped run; run_without(k, sched, seed, desc) -> the same of the run without barrier k of every period under one schedule.  A
    knocked-out barrier is still counted, so the counts do not change.  For every `needed` barrier the run without it differs from the
    shipped run under some schedule; for every other one it is bit-identical under all of them."""
    base, bars = run_base()
    order = sorted(SCHEDULES, key=lambda s: s[0] != DESC)       # `descending` first: it is the one that shows most
    for k, entry in enumerate(table):
        differs = None
        for sched, seed, desc in order:
            got, b = run_without(k, sched, seed, desc)
            assert b == bars, (label, k, b, bars)
            if not same(got, base):
                differs = (sched, seed, desc)
                break
        print(f"{label} barrier {k}: {'differs under ' + str(differs) if differs else 'bit-identical under all schedules'}")
        if entry == "needed":
            assert differs, f"{label}: barrier {k} is entered as needed, but no schedule shows a difference without it"
        else:
            assert not differs, f"{label}: barrier {k} is entered as redundant, but schedule {differs} differs without it"

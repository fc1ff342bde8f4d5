"""The transform cases of tests/test_probes_gpu.py: every transform kernel of tests/kernel_inventory.py through the calls its entry
names, with the number of applications k on the `multiple` paths.  Kept apart from the GPU module so that the CPU suite can check
tests/accuracy_ratchet.json against exactly these ids (tests/test_accuracy_ratchet.py) without importing anything of the GPU's.

A case id is "<kind>-N<n>-<fwd|inv>[-noreorder]-k<k>"; kinds:
  ct_external          SMFFT_DIT_external (and SMFFT_DIT_external_occ3 at N = 4096 natural order)
  ct_multiple          SMFFT_DIT_multiple: the in-LDS path (path 1), k applications per slot
  ct_multiple_unfused  SMFFT_DIT_multiple_unfused: one image load and store per application (path 2); N = 32 and N = 64 without
                       reorder are the lane engines
  st_external          FFT_GPU_external (inverse: the Stockham program; forward: the extension on the CT kernels)
  st_multiple          FFT_GPU_multiple (inverse) and the forward extension on SMFFT_DIT_multiple
  r2c_* / c2r_*        FFT_GPU_R2C_C2R_external / _multiple, N reals <-> N / 2 packed complex
  dif                  SMFFT_DIF_external: natural order in, bit-reversed spectrum out
  large                large_c2c of libsmfft_large.so (smfft_amd.large.c2c): N = 8192 and 16384, natural order, k = 1, a persistent
                       grid of G = smfft_amd.large.grid(N) workgroups over the batch"""
import math
from collections import namedtuple

C2C_SIZES = [32, 64, 128, 256, 512, 1024, 2048, 4096]
R2C_SIZES = [512, 1024, 2048, 4096]
LARGE_SIZES = [8192, 16384]
# the kernels path 2 has of its own (everything else on path 2 is the path-1 kernel): (N, reorder)
PERCALL_KERNELS = [(n, 1) for n in C2C_SIZES] + [(32, 0), (64, 0)]


def lane_engine(n, reo):
    """the register engines that flip sign bits on odd applications (smfft_engine.hpp, PairEngine32 / QuadEngine64)"""
    return n == 32 or (n == 64 and not reo)


class Case(namedtuple("Case", "kind n inv reo k")):
    __slots__ = ()

    @property
    def id(self):
        return f"{self.kind}-N{self.n}-{'inv' if self.inv else 'fwd'}{'' if self.reo else '-noreorder'}-k{self.k}"

    @property
    def real_in(self):
        return self.kind.startswith("r2c")

    @property
    def real_out(self):
        return self.kind.startswith("c2r")

    @property
    def multiple(self):
        return "multiple" in self.kind


def _ks(n, reo):
    return (1, 2, 3) if lane_engine(n, reo) else (1, 2)


def _cases():
    out = []
    for n in C2C_SIZES:
        for inv in (0, 1):
            for reo in (1, 0):
                out.append(Case("ct_external", n, inv, reo, 1))
                out += [Case("ct_multiple", n, inv, reo, k) for k in _ks(n, reo)]
            out.append(Case("st_external", n, inv, 1, 1))
            out += [Case("st_multiple", n, inv, 1, k) for k in (1, 2)]
            out.append(Case("dif", n, inv, 0, 1))
    for n, reo in PERCALL_KERNELS:
        for inv in (0, 1):
            out += [Case("ct_multiple_unfused", n, inv, reo, k) for k in _ks(n, reo)]
    for n in R2C_SIZES:
        out += [Case("r2c_external", n, 0, 1, 1), Case("c2r_external", n, 1, 1, 1)]
        out += [Case("r2c_multiple", n, 0, 1, k) for k in (1, 2)] + [Case("c2r_multiple", n, 1, 1, k) for k in (1, 2)]
    for n in LARGE_SIZES:
        out += [Case("large", n, inv, 1, 1) for inv in (0, 1)]
    return out


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES)

REL_L2_TOL = 5e-7          # the library's per-FFT bound (oracle/np_reference.py), grown as sqrt(k) over k applications
RATCHET_SLACK = 1.25       # a measured figure may exceed its committed entry by at most this factor


def probe_ceiling(n, k):
    """the A1 per-element ceiling, relative to max |ref| of the row (tests/test_probes_gpu.py, test_dft_matrix_probe)"""
    return k * 3 * (math.log2(n) + 2) * 2.0 ** -24


def gauss_bound(k):
    return REL_L2_TOL * math.sqrt(k)


# ---------------------------------------------------------------------------------------------------- the header's device functions
"""HEADER_CASES: the cases of tests/test_device_probes_gpu.py -- every function of the header-only device API (tests/
device_function_inventory.py) through the test entry points that already drive it: the dc_* launchers of tests/hip/device_contract.hip
(libsmfft_device_contract{,_unfused_io,_no_phases,_no_pairs,_nreuses3}.so), the smfft_example_* entries of examples/
(libsmfft_examples{,_wave64small,_unfused_io,_no_phases,_no_pairs}.so).  A case id is
"hdr_<func>-<build>-N<n>-<fwd|inv>[-noreorder]-k<k>"; for the R2C / C2R functions N is the complex length L (real length 2L)."""

# func -> (entry point, the inventory functions it runs, (IN_REGS, OUT_REGS) of the quarter_fft call behind it or None for the tiled
# engine, which none of the switches reaches)
HEADER_FUNCS = {
    "ct":                  ("smfft_example_reference_shape_ct which=0", ["do_SMFFT_CT_DIT"], (False, False)),
    "ct_wave64":           ("smfft_example_reference_shape_ct which=2", ["do_SMFFT_CT_DIT"], (False, False)),
    "ct_ext":              ("smfft_example_reference_shape_ct which=1", ["SMFFT_DIT_external", "do_SMFFT_CT_DIT_registers_out"], (True, True)),
    "ct_ext_wave64":       ("smfft_example_reference_shape_ct which=3", ["SMFFT_DIT_external"], (False, False)),
    "ct_times":            ("smfft_example_reference_shape_ct_times", ["do_SMFFT_CT_DIT"], (False, False)),
    "ct_registers":        ("dc_ct_registers", ["do_SMFFT_CT_DIT_registers"], (True, True)),
    "ct_multiple":         ("dc_ct_multiple wave64=0", ["SMFFT_DIT_multiple", "do_SMFFT_CT_DIT"], (False, False)),
    "ct_multiple_wave64":  ("dc_ct_multiple wave64=1", ["SMFFT_DIT_multiple", "do_SMFFT_CT_DIT"], (False, False)),
    "st_mk6":              ("dc_stockham fn=0", ["do_FFT_Stockham_mk6"], (False, False)),
    "st_c2c":              ("dc_stockham fn=1, 2", ["do_FFT_Stockham_C2C"], (False, False)),
    "st_registers":        ("dc_stockham_registers fn=0", ["do_FFT_Stockham_C2C_registers"], (True, True)),
    "st_registers_out":    ("dc_stockham_registers fn=1", ["do_FFT_Stockham_C2C_registers_out"], (True, True)),
    "st_ext":              ("dc_fft_gpu_external (N <= 128), smfft_example_reference_shape_st", ["FFT_GPU_external", "do_FFT_Stockham_C2C_registers_out"], (True, True)),
    "st_multiple":         ("dc_fft_gpu_multiple", ["FFT_GPU_multiple", "do_FFT_Stockham_mk6"], (False, False)),
    "rc":                  ("dc_stockham fn=3, 4", ["do_FFT_Stockham_R2C_C2R"], (False, False)),
    "rc_ext":              ("smfft_example_reference_shape_rc", ["FFT_GPU_R2C_C2R_external"], None),
    "rc_multiple":         ("dc_rc_multiple", ["FFT_GPU_R2C_C2R_multiple", "do_FFT_Stockham_R2C_C2R"], (False, False)),
    "tiled_ct":            ("dc_tiled_ct", ["smfft::tiled::do_SMFFT_CT_DIT"], None),
    "tiled_mk6":           ("dc_tiled fn=0", ["smfft::tiled::do_FFT_Stockham_mk6"], None),
    "tiled_c2c":           ("dc_tiled fn=1, 2", ["smfft::tiled::do_FFT_Stockham_C2C"], None),
    "tiled_rc":            ("dc_tiled fn=3, 4", ["smfft::tiled::do_FFT_Stockham_R2C_C2R"], None),
    "dif":                 ("smfft_example_dif_ct which=0", ["do_SMFFT_CT_DIF"], None),
    "dif_registers":       ("smfft_example_dif_ct which=1", ["do_SMFFT_CT_DIF_registers"], None),
    "dif_wave64":          ("smfft_example_dif_ct which=2", ["do_SMFFT_CT_DIF"], None),
}
SMALL_SIZES = [32, 64, 128]
REG_SIZES = [256, 512, 1024, 2048, 4096]
RC_L = [32, 64, 128, 256, 512, 1024, 2048]
HEADER_BUILDS = ["default", "wave64small", "unfused_io", "no_phases", "no_pairs"]
# the switch builds exist for the entry points of these files (smfft_amd/csrc/Makefile); the `multiple` kernels run in the NREUSES = 3
# build of device_contract.hip only, and the DIF entries in the default build of the examples only
SWITCH_FUNCS = {
    "wave64small": {"ct", "ct_ext"},                                                      # examples/reference_shape_kernel.hip
    "unfused_io": {"ct_ext", "st_ext", "rc_ext"},
    "no_phases": {"ct", "ct_wave64", "ct_ext", "ct_ext_wave64", "ct_registers", "st_mk6", "st_c2c", "st_registers", "st_registers_out",
                  "st_ext", "rc", "rc_ext"},
    "no_pairs": {"ct", "ct_ext", "ct_registers", "st_mk6", "st_c2c", "st_registers", "st_registers_out", "st_ext", "rc", "rc_ext"},
}


def _rc_ext_regs(inv):
    """FFT_GPU_R2C_C2R_external (fused): R2C runs quarter_fft with its inputs in registers, C2R with its results in registers"""
    return (True, False) if not inv else (False, True)


def switch_changes(build, func, n, inv, reo):
    """whether the header switch of `build` changes the code the case runs -- the conditions of include/smfft/SM_FFT_parameters.hpp
    (SMFFT_WAVE64_SMALL) and include/smfft/smfft_device_functions.hpp (SMFFT_CONTRACT_FUSED_IO in the two-argument kernels; kPhases,
    kPairs, kPairsHead in quarter_fft):
      wave64small  the upstream class names of N <= 128 become 64-thread blocks (SMFFT_SMALL_BLOCK_LENGTH 128 -> 256)
      unfused_io   SMFFT_DIT_external: the LDS-free lane ladder of the 32-thread blocks of N <= 128 (not N = 128 natural order, kStagedSmall,
                   nor the _wave64 classes) and the registers form of N >= 256; FFT_GPU_external and FFT_GPU_R2C_C2R_external: every length
      no_phases    kPhases: the N = 64 / 128 one-trip form (blocks <= 64 threads), N = 256 in one wave, the lane head / middle of
                   N >= 512, the last phase of N >= 2048, kStagedSmall; N = 32 runs the lane ladder or the LDS form either way
      no_pairs     kPairs (natural order, N = 512 / 1024, results to LDS) and kPairsHead (natural order, N = 2048, inputs from LDS)"""
    if func not in SWITCH_FUNCS[build]:
        return False
    if build == "wave64small":
        return n <= 128
    if build == "unfused_io":
        return func != "ct_ext" or n >= 256 or not (n == 128 and reo)
    if build == "no_phases":
        return n >= 64
    regs = _rc_ext_regs(inv) if func == "rc_ext" else HEADER_FUNCS[func][2]
    if func == "ct_ext":
        regs = (True, True) if n >= 256 else (False, False)
    if func == "st_ext":
        regs = (True, True)
    in_regs, out_regs = regs
    return bool(reo) and ((n in (512, 1024) and not out_regs) or (n == 2048 and not in_regs))


class HCase(namedtuple("HCase", "func build n inv reo k")):
    __slots__ = ()

    @property
    def id(self):
        return f"hdr_{self.func}-{self.build}-N{self.n}-{'inv' if self.inv else 'fwd'}{'' if self.reo else '-noreorder'}-k{self.k}"

    @property
    def rc(self):
        return self.func in ("rc", "rc_ext", "rc_multiple", "tiled_rc")

    def as_lib(self):
        """the same transform as a library Case (kind r2c_hdr / c2r_hdr / dif / ct_hdr, N the library's length): its fp64
        statement, A1 / A2 batches and seeds are tests/test_probes_gpu.py's"""
        if self.rc:
            kind = "c2r_hdr" if self.inv else "r2c_hdr"
        else:
            kind = "dif" if self.func.startswith("dif") else "ct_hdr"
        return Case(kind, self.length, self.inv, self.reo, self.k)

    @property
    def length(self):
        """the transform's length in the library's terms: real length 2L for R2C / C2R, N otherwise"""
        return 2 * self.n if self.rc else self.n

    @property
    def wave64(self):
        return self.func.endswith("_wave64")

    @property
    def per_block(self):
        """transforms per block of the entry's launch (the reference's shape: fft_length / N; tiled: 4096 / N)"""
        if self.func.startswith("tiled"):
            return 4096 // self.n
        if self.func in ("ct", "ct_ext", "ct_times", "ct_multiple", "dif") and self.n <= 128:
            return (256 if self.build == "wave64small" else 128) // self.n
        if self.wave64:
            return 256 // self.n
        return 1


def _header_cases():
    out = []

    def add(func, sizes, dirs, orders, k=1):
        for build in HEADER_BUILDS:
            for n in sizes:
                for inv in dirs:
                    for reo in orders:
                        if build == "default" or (func in SWITCH_FUNCS[build] and switch_changes(build, func, n, inv, reo)):
                            out.append(HCase(func, build, n, inv, reo, k))

    both, orders = (0, 1), (1, 0)
    for func in ("ct", "ct_ext"):
        add(func, C2C_SIZES, both, orders)
    for func in ("ct_wave64", "ct_ext_wave64"):
        add(func, SMALL_SIZES, both, orders)
    add("ct_times", [64, 256, 2048], (0,), orders, k=2)
    add("ct_registers", REG_SIZES, both, orders)
    add("ct_multiple", C2C_SIZES, both, orders, k=3)
    add("ct_multiple_wave64", SMALL_SIZES, both, orders, k=3)
    add("st_mk6", C2C_SIZES, (1,), (1,))
    for func in ("st_c2c", "st_registers", "st_registers_out"):
        add(func, C2C_SIZES, both, (1,))
    add("st_ext", C2C_SIZES, (1,), (1,))
    add("st_multiple", C2C_SIZES, (1,), (1,), k=3)
    add("rc", RC_L, both, (1,))
    add("rc_ext", [256, 512, 1024, 2048], both, (1,))
    add("rc_multiple", RC_L, both, (1,), k=3)
    add("tiled_ct", C2C_SIZES, both, orders)
    add("tiled_mk6", C2C_SIZES, (1,), (1,))
    add("tiled_c2c", C2C_SIZES, both, (1,))
    add("tiled_rc", RC_L, both, (1,))
    add("dif", C2C_SIZES, both, (0,))
    add("dif_registers", REG_SIZES, both, (0,))
    add("dif_wave64", SMALL_SIZES, both, (0,))
    return out


HEADER_CASES = _header_cases()
assert len({c.id for c in HEADER_CASES}) == len(HEADER_CASES)
assert not {c.id for c in HEADER_CASES} & {c.id for c in CASES}

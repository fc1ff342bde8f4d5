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

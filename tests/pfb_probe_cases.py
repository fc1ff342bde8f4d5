"""The tap-matrix probe cases of tests/test_pfb_probes_gpu.py: the twenty kernels of libsmfft_pfb.so and libsmfft_pfb_real.so (tests/
pfb_inventory.py), one impulse per frame.  Kept apart from the GPU module, like tests/probe_cases.py, so that the CPU suite can check
tests/pfb_accuracy_ratchet.json against exactly these ids (tests/test_pfb_accuracy_ratchet.py) without importing anything of the GPU's.

A case id is "<pfb|pfb_real>-N<n>-P<p>-<all|sub>-<complex|power>".  A chunk is W = N complex samples (pfb) or W = 2N real samples
(pfb_real); the case's stream holds, for every position n_i of positions(), a single 1.0 at position n_i of chunk P i + P - 1, so
frame f = P i + r sees exactly h[(P - 1 - r) W + n_i] at position n_i and nothing else.
  all   every position of the chunk, complex mode, one P per N (ALL_TAPS; no case has more than 2^25 output elements); N = 256 also with
        P = 1 and P = 32, in both modes
  sub   P = 32, both modes, 256 positions: in float2 units n = u + T q (T = N / 16: thread index u, register index q), position i takes
        u = i mod T and q = (i div T + i) mod 16 -- every u and every q, no (u, q) twice --, and for the real bank the sample of the
        pair alternates as ((i >> 1) ^ i) & 1

inputs(case) builds the stream and the taps -- uniform(0.5, 1) with a random sign, in fp32, so that every tap has a value of its own and
a wrong tap index is a wrong element --, expected(case, ...) is the closed form of the output in fp64: h W_N^{n k} for the complex
bank, h W_2N^{m k}, 0 <= k <= N, for the real bank, the root of unity read from one fp64 table at the integer product mod W.
tests/test_pfb_accuracy_ratchet.py holds it to tools/pfb_model.py and tools/pfb_real_model.py."""
from collections import namedtuple

import numpy as np

from tests import probe_cases as pc

SIZES = [256, 512, 1024, 2048, 4096]
ALL_TAPS = {"pfb": dict(zip(SIZES, (3, 2, 4, 2, 2))), "pfb_real": dict(zip(SIZES, (3, 2, 2, 2, 1)))}
SUB_POSITIONS = 256
MAX_OUTPUT_ELEMENTS = 1 << 25


class Case(namedtuple("Case", "bank n p tag power")):
    __slots__ = ()

    @property
    def id(self):
        return f"{self.bank}-N{self.n}-P{self.p}-{self.tag}-{'power' if self.power else 'complex'}"

    @property
    def real(self):
        return self.bank == "pfb_real"

    @property
    def chunk(self):
        """W: samples per chunk = the transform's length"""
        return 2 * self.n if self.real else self.n

    def positions(self):
        """the n_i: sample positions inside a chunk, 0 <= n_i < W"""
        if self.tag == "all":
            return list(range(self.chunk))
        t = self.n // 16
        out = []
        for i in range(SUB_POSITIONS):
            n = i % t + t * ((i // t + i) % 16)
            out.append(2 * n + (((i >> 1) ^ i) & 1) if self.real else n)
        return out

    @property
    def frames(self):
        return self.p * len(self.positions())

    @property
    def ceiling(self):
        """the per-element bound, relative to |h| of the frame (h^2 in power mode): the transform probes' ceiling at the transform's
        length (the Hermitian step of the real bank is its `+ 2`); in power mode | |y + d|^2 - |y|^2 | <= 2 |y| |d| + |d|^2 plus the two
        roundings of fma(x, x, y y)"""
        c = pc.probe_ceiling(self.chunk, 1)
        return 2 * c + 2.0 ** -22 if self.power else c


def inputs(case):
    """(x, h, pos): the stream (1, (P I + P - 1) W) with its I impulses, the P W taps, the positions as an array"""
    W, P = case.chunk, case.p
    pos = np.asarray(case.positions(), np.int64)
    rng = np.random.default_rng([case.real, case.n, case.p, len(pos)])
    h = (rng.uniform(0.5, 1.0, P * W) * rng.choice([-1.0, 1.0], P * W)).astype(np.float32)
    x = np.zeros((1, (P * len(pos) + P - 1) * W), np.float32 if case.real else np.complex64)
    x[0, (P * np.arange(len(pos)) + P - 1) * W + pos] = 1
    return x, h, pos


def frame_taps(case, h, pos, f):
    """(n, h_f) of the frames f: the position of the one nonzero sample frame f sees, and the tap it meets, h[(P - 1 - f mod P) W + n]"""
    f = np.asarray(f, np.int64)
    n = pos[f // case.p]
    return n, np.asarray(h, np.float64)[(case.p - 1 - f % case.p) * case.chunk + n]


def expected(case, h, pos, f):
    """the spectra of the frames f in fp64: (len(f), N) complex128 for the complex bank, (len(f), N + 1) for the real bank (np.fft.rfft
    layout)"""
    W = case.chunk
    n, hf = frame_taps(case, h, pos, f)
    table = np.exp(-2j * np.pi * np.arange(W) / W)
    k = np.arange(case.n + 1 if case.real else case.n, dtype=np.int64)
    return hf[:, None] * table[(n[:, None] * k) & (W - 1)]


def _cases():
    out = []
    for bank in ("pfb", "pfb_real"):
        for n in SIZES:
            out.append(Case(bank, n, ALL_TAPS[bank][n], "all", 0))
            out += [Case(bank, n, 32, "sub", power) for power in (0, 1)]
        out += [Case(bank, 256, p, "all", power) for p in (1, 32) for power in (0, 1)]
    return out


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES)

#!/usr/bin/env python3
"""NumPy model of the decimation-in-frequency ladder (include/smfft/smfft_dif.hpp: dif_ladder, DifPlan) -- the transpose of the
no-reorder DIT ladder: natural order in, bit-reversed spectrum out.

Replays, thread by thread, what a block of the reference's shape does: the four registers of every thread, the twiddles it fetches
(indices into the 4096-entry table), the swizzled LDS image between passes (quarter_swizzle, the DIT ladder's), and counts the LDS
accesses and their bank-conflict cycles with the gfx950 rules of tools/quarter_swizzle.py (MI355X_MICROARCH.md, LDS): ds_read_b64
in two groups of 32 lanes on 32 float2 banks, ds_write_b64 in four groups of 16 lanes on 16 float2 banks, never under 6 cycles.
    python tools/dif_ladder_model.py            check against numpy.fft for every length and direction + the LDS table
The header's index functions (DifPlan::element / twiddle_index, quarter_swizzle) must equal element() / twiddle_index() /
quarter_swizzle.product_swizzle here (tests/test_dif_cpu.py compiles them on the host and compares)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from quarter_swizzle import product_swizzle  # noqa: E402

SIZES = (32, 64, 128, 256, 512, 1024, 2048, 4096)


def ilog2(x):
    return x.bit_length() - 1


def bitrev_indices(n):
    bits = ilog2(n)
    return np.array([int(format(j, f"0{bits}b")[::-1], 2) for j in range(n)], dtype=np.int64)


class Plan:
    """DifPlan<N>: pass j = 0 .. passes-1; an odd log2 N starts with a radix-2 pass, then quarter spans 4^(quads-1) ... 1"""

    def __init__(self, n):
        self.n, self.bits = n, ilog2(n)
        self.odd = self.bits & 1
        self.quads = self.bits // 2
        self.passes = self.quads + self.odd

    def radix2(self, j):
        return self.odd and j == 0

    def span(self, j):
        return 1 << (2 * (self.quads - 1 - (j - self.odd)))

    def element(self, j, t, m):
        if self.radix2(j):
            return t + m * (self.n // 4)
        L = self.span(j)
        return (t // L) * 4 * L + t % L + m * L

    def twiddle_index(self, j, t):
        """index into W_4096^i of w2 = W_4L^(t mod L) (radix-2 pass: W_N^t); -1: none (L = 1)"""
        if self.radix2(j):
            return (t * (4096 // self.n)) & 4095
        L = self.span(j)
        return -1 if L == 1 else ((t % L) * (4096 // (4 * L))) & 4095

    def crosses_waves(self, j):
        return self.n > 256 and (self.radix2(j) or self.span(j) >= 256)


def block_threads(n, wave64=False):
    """threads of a block in the reference's shape: 32 (or 64: the _wave64 classes) for N <= 128, N / 4 above"""
    return (64 if wave64 else 32) if n <= 128 else n // 4


def transform(n, direction, x, wave64=False, log=None, contract=False):
    """x: (batch, n) complex with batch a multiple of the block's transforms; returns the DIF output (batch, n).
    log: list that collects (kind, [physical LDS address per thread of the block]) of every LDS instruction (one block)."""
    plan = Plan(n)
    q = n // 4
    threads = block_threads(n, wave64)
    per_block = threads * 4 // n
    x = np.asarray(x, dtype=np.complex128)
    batch = x.shape[0]
    assert batch % per_block == 0
    blocks = x.reshape(batch // per_block, per_block * n)              # one row per block: its transforms back to back
    tid = np.arange(threads)
    f, t = tid // q, tid % q
    sign = 1.0 if direction else -1.0
    lds = np.full(blocks.shape, np.nan + 0j)

    def note(kind, addr):
        if log is not None:
            log.append((kind, [int(a) for a in addr]))

    def twiddle(j):
        idx = np.array([plan.twiddle_index(j, int(u)) for u in t])
        return np.where(idx >= 0, np.exp(sign * 2j * np.pi * np.maximum(idx, 0) / 4096), 1.0)

    if contract:                                    # the caller's natural layout in s
        lds[:] = blocks
    e = []
    for m in range(4):
        addr = f * n + t + m * q
        if contract:
            note("r", addr)
        e.append(blocks[:, addr].copy())
    for j in range(plan.passes):
        if j > 0:
            for m in range(4):
                addr = np.array([product_swizzle(int(a)) for a in f * n + np.array([plan.element(j, int(u), m) for u in t])])
                note("r", addr)
                e[m] = lds[:, addr].copy()
        w = twiddle(j)
        if plan.radix2(j):
            a0, a1 = e[0] + e[2], e[1] + e[3]
            b0, b1 = (e[0] - e[2]) * w, (e[1] - e[3]) * w
            e = [a0, a1, b0, b1 * (1j * sign)]
        else:
            s0, d0, s1 = e[0] + e[2], e[0] - e[2], e[1] + e[3]
            d1 = (e[1] - e[3]) * (1j * sign)             # (-+i)(e1 - e3): the forward transform's W_4 = -i
            e = [s0 + s1, (s0 - s1) * w ** 2, (d0 + d1) * w, (d0 - d1) * w ** 3]
        if j + 1 < plan.passes:
            for m in range(4):
                addr = np.array([product_swizzle(int(a)) for a in f * n + np.array([plan.element(j, int(u), m) for u in t])])
                note("w", addr)
                lds[:, addr] = e[m]
    out = np.empty_like(blocks)
    for m in range(4):
        addr = f * n + 4 * t + m                         # the last pass's positions: the bit-reversed result
        if contract:
            note("w", addr)
        out[:, addr] = e[m]
    return out.reshape(batch, n)


def reference(n, direction, x):
    x = np.asarray(x, dtype=np.complex128)
    spec = np.fft.ifft(x, axis=-1) * n if direction else np.fft.fft(x, axis=-1)
    return spec[..., bitrev_indices(n)]


def access_cycles(kind, addr):
    """LDS cycles of one instruction of a block, summed over its waves (tools/quarter_swizzle.py's rules)"""
    total = 0
    for w0 in range(0, len(addr), 64):
        wave = addr[w0:w0 + 64]
        group, banks, floor = (32, 32, 0) if kind == "r" else (16, 16, 6)
        cycles = 0
        for g0 in range(0, len(wave), group):
            load = {}
            for a in set(wave[g0:g0 + group]):
                load[a % banks] = load.get(a % banks, 0) + 1
            cycles += max(load.values())
        total += max(floor, cycles)
    return total


def ideal_cycles(kind, addr):
    waves = (len(addr) + 63) // 64
    return waves * (2 if kind == "r" else 6) if len(addr) > 32 else waves * (1 if kind == "r" else 6)


def lds_report(n, contract=False, wave64=False):
    """(reads, writes per thread, cycles per block, conflict-free cycles per block, workgroup barriers)"""
    log = []
    threads = block_threads(n, wave64)
    transform(n, 0, np.zeros((threads * 4 // n, n)), wave64=wave64, log=log, contract=contract)
    plan = Plan(n)
    reads = sum(k == "r" for k, _ in log)
    writes = sum(k == "w" for k, _ in log)
    cycles = sum(access_cycles(k, a) for k, a in log)
    ideal = sum(ideal_cycles(k, a) for k, a in log)
    barriers = sum(plan.crosses_waves(j) for j in range(plan.passes - 1)) + (1 if contract and n > 256 else 0)
    return reads, writes, cycles, ideal, barriers


def check(verbose=True):
    rng = np.random.default_rng(7)
    worst = 0.0
    for n in SIZES:
        for direction in (0, 1):
            for wave64 in ((False, True) if n <= 128 else (False,)):
                per_block = block_threads(n, wave64) * 4 // n
                x = rng.standard_normal((2 * per_block, n)) + 1j * rng.standard_normal((2 * per_block, n))
                got = transform(n, direction, x, wave64=wave64)
                err = np.max(np.abs(got - reference(n, direction, x))) / np.max(np.abs(reference(n, direction, x)))
                worst = max(worst, err)
                assert err < 1e-12, (n, direction, wave64, err)
    if verbose:
        print(f"DIF ladder == fft(x)[bitrev] for N = 32 ... 4096, both directions (worst relative error {worst:.1e})")


def main():
    check()
    print(f"{'N':>5s} {'form':9s} {'ds_read':>7s} {'ds_write':>8s} {'LDS cycles':>10s} {'conflict-free':>13s} {'barriers':>8s}   (per thread / per block of the reference's shape)")
    for n in SIZES:
        for contract in (False, True):
            if not contract and n < 256:
                continue
            r, w, c, i, b = lds_report(n, contract)
            print(f"{n:5d} {'contract' if contract else 'registers':9s} {r:7d} {w:8d} {c:10d} {i:13d} {b:8d}")


if __name__ == "__main__":
    main()

"""The fp64 model of the polyphase filter bank channelizer for N = 8192 / 16384 channels (include/smfft_large_pfb.h,
include/smfft/smfft_large_pfb.hpp).

  pfb, pfb_direct, scale, frames, Plan     tools/pfb_model.py's: the definition does not depend on N, and smfft::PfbPlan is used unchanged
                                           (its tiles and runs belong to the small banks and are not used here)
  Schedule                                 smfft::large::LargePfbSchedule, line by line
  replay(plan, sched)                      what every thread of a launch loads and stores: element addresses per (pair, tap)
  leakage(N, P)                            a unit tone at channel 100.37 through the Hamming prototype: (power outside channel 100) / (power in it)

The CPU test compiles the header's struct for the host and compares it with Schedule; the host run and the GPU tests use pfb() as their
reference.
    python tools/large_pfb_model.py        # the two forms of the definition, the replay and the leakage figures
"""
import numpy as np

import pfb_model as pm

SIZES = (8192, 16384)
STRIDE, XCD_BLOCKED = 1, 2
pfb, pfb_direct, scale, frames, Plan = pm.pfb, pm.pfb_direct, pm.scale, pm.frames, pm.Plan


class Schedule:
    """smfft::large::LargePfbSchedule"""

    def __init__(self, pairs, grid, form):
        self.pairs, self.grid, self.form = pairs, grid, form

    @staticmethod
    def make(pairs, cap, form):
        g = min(pairs, cap)
        if form == 2:
            if g >= 8:
                g -= g % 8
            else:
                form = 1
        return Schedule(pairs, g, form)

    def rounds(self):
        return -(-self.pairs // self.grid)

    def slot(self, b):
        return (b % 8) * (self.grid // 8) + b // 8 if self.form == 2 else b

    def pair_of(self, b, t):
        g = t * self.grid + self.slot(b)
        return g if g < self.pairs else -1

    def pairs_of(self, b):
        """the pairs of workgroup b in the order the kernel visits them (the loop of the kernel: t = 0, 1, ... while t grid < pairs)"""
        out, t = [], 0
        while t * self.grid < self.pairs:
            g = self.pair_of(b, t)
            if g >= 0:
                out.append(g)
            t += 1
        return out


def positions(N):
    """(T, 16): the element numbers u + T q that thread u holds at the loads and at the store"""
    T = N // 16
    return np.arange(T)[:, None] + T * np.arange(16)[None, :]


def replay(plan, sched):
    """The kernel's loops, thread by thread (vectorised over the T threads and 16 registers): returns
    loads  -- list of (pair, stream, int64 array (P, T, 16)) signal element addresses read for the pair,
    stores -- int64 array of every output element address stored, in issue order,
    taps   -- the largest coefficient index read."""
    N, P = plan.N, plan.P
    pos = positions(N).astype(np.int64)
    loads, stores, taps = [], [], -1
    for b in range(sched.grid):
        for g in sched.pairs_of(b):
            addr = plan.input_offset(g) + np.arange(P, dtype=np.int64)[:, None, None] * N + pos[None]
            taps = max(taps, int((P - 1) * N + pos.max()))
            loads.append((g, plan.stream_of(g), addr))
            stores.append((plan.output_offset(g) + pos).reshape(-1))
    return loads, (np.concatenate(stores) if stores else np.empty(0, np.int64)), taps


def check_replay(plan, sched):
    """every output element stored exactly once, every load inside its own stream's [0, (F + P - 1) N), every pair's loads its window"""
    F, N, P, L, C = plan.frames(), plan.N, plan.P, plan.L, plan.C
    loads, stores, taps = replay(plan, sched)
    assert np.array_equal(np.sort(stores), np.arange(C * F * N)), "every output element exactly once"
    assert taps == P * N - 1
    assert sorted(g for g, _, _ in loads) == list(range(C * F)), "every pair exactly once"
    for g, c, addr in loads:
        assert addr.min() >= c * L and addr.max() < c * L + (F + P - 1) * N, (g, c)
        f = g - c * F
        assert np.array_equal(np.sort(addr.reshape(P, N), axis=1), c * L + (f + np.arange(P))[:, None] * N + np.arange(N)[None, :]), g
    return len(loads)


def tone(N, length, channel=100.37, amplitude=1.0):
    return amplitude * np.exp(2j * np.pi * channel * np.arange(length) / N)


def hamming_prototype(N, P):
    M = P * N
    m = np.arange(M, dtype=np.float64)
    return np.sinc((m - (M - 1) / 2) / N) * np.hamming(M)


def leakage_of(power, channel):
    """(power outside `channel`) / (power in it), per spectrum"""
    power = np.asarray(power, np.float64)
    return (power.sum(axis=-1) - power[..., channel]) / power[..., channel]


def leakage(N, P, channel=100.37):
    return float(leakage_of(pfb(tone(N, P * N, channel), hamming_prototype(N, P), N, power=True)[0, 0], int(round(channel))))


if __name__ == "__main__":
    rng = np.random.default_rng(0)
    N, P, C, L = 256, 3, 2, 6 * 256 + 17          # the definition is the same at every N: the O(P N^2) form at a small one
    x, h = rng.standard_normal((C, L)) + 1j * rng.standard_normal((C, L)), rng.standard_normal(P * N)
    a, b = pfb(x, h, N), pfb_direct(x, h, N)
    print(f"two forms of the definition, N={N}: max |a - b| / max |b| = {np.max(np.abs(a - b)) / np.max(np.abs(b)):.2e}")
    for N in SIZES:
        plan = Plan(12 * N + 5, N, 3, 3)
        for form, cap in ((1, 7), (2, 8), (2, 20)):
            sched = Schedule.make(plan.pairs(), cap, form)
            print(f"N={N} pairs={plan.pairs()} form {sched.form} grid {sched.grid}: replay of {check_replay(plan, sched)} pairs: stores once, loads inside the window")
        print(f"N={N}: leakage of a tone at channel 100.37: " + ", ".join(f"P={P}: {leakage(N, P):.3g}" for P in (1, 2, 4, 8, 16, 32)))

"""The fp64 model of the polyphase filter bank channelizer (include/smfft_pfb.h) and of its plan (smfft_amd/csrc/smfft_pfb.hpp).

  pfb(x, h, N)          the definition's first form: frames by sliding_window_view, weighted sum over the P branches, np.fft.fft
  pfb_direct(x, h, N)   the second form: the O(P N^2) direct sum  sum_m h[m] x[f N + m] exp(-2 pi i k m / N)
  Plan                  PfbPlan, line by line
  replay(plan, G, R)    what every thread of a launch on a grid of G workgroups loads and stores: element addresses per (pair, tap)

The CPU test compiles the header for the host and compares it with Plan; the GPU tests use pfb() as their reference."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view


def frames(L, N, P):
    return max(L // N - P + 1, 0)


def pfb(x, h, N, power=False):
    """x: (C, L) complex, h: P N real -> (C, F, N) complex128 (or |.|^2 as float64)"""
    x = np.atleast_2d(np.asarray(x, np.complex128))
    h = np.asarray(h, np.float64)
    P = h.size // N
    assert h.size == P * N and P >= 1
    C, L = x.shape
    F = frames(L, N, P)
    if F == 0:
        return np.empty((C, 0, N), np.float64 if power else np.complex128)
    blocks = x[:, :(F + P - 1) * N].reshape(C, F + P - 1, N)
    win = sliding_window_view(blocks, P, axis=1)          # (C, F, N, P): win[c, f, n, p] = x_c[(f + p) N + n]
    w = np.einsum("cfnp,pn->cfn", win, h.reshape(P, N))
    y = np.fft.fft(w, axis=-1)
    return y.real ** 2 + y.imag ** 2 if power else y


def pfb_direct(x, h, N):
    x = np.atleast_2d(np.asarray(x, np.complex128))
    h = np.asarray(h, np.float64)
    M = h.size
    P = M // N
    C, L = x.shape
    F = frames(L, N, P)
    k, m = np.arange(N)[:, None], np.arange(M)[None, :]
    E = np.exp(-2j * np.pi * ((k * m) % N) / N)           # (N, M)
    y = np.empty((C, F, N), np.complex128)
    for c in range(C):
        for f in range(F):
            y[c, f] = E @ (h * x[c, f * N:f * N + M])
    return y


def scale(x, h, N):
    """s[c, f, n] = sum_p |h[p N + n]| |x_c[(f + p) N + n]|: what the fp32 accumulation rounds at (the tolerances' denominator)"""
    return pfb_weights_only(np.abs(np.atleast_2d(x)), np.abs(np.asarray(h, np.float64)), N)


def pfb_weights_only(x, h, N):
    x = np.atleast_2d(np.asarray(x))
    P = h.size // N
    C, L = x.shape
    F = frames(L, N, P)
    blocks = x[:, :(F + P - 1) * N].reshape(C, F + P - 1, N)
    return np.einsum("cfnp,pn->cfn", sliding_window_view(blocks, P, axis=1), h.reshape(P, N))


class Plan:
    """smfft::PfbPlan"""

    def __init__(self, L, N, P, C):
        self.L, self.N, self.P, self.C = L, N, P, C

    def frames(self):
        return frames(self.L, self.N, self.P)

    def pairs(self):
        return self.frames() * self.C

    def per_tile(self):
        return 4096 // self.N

    def tiles(self):
        return -(-self.pairs() // self.per_tile())

    def pair_of(self, tile, j):
        g = tile * self.per_tile() + j
        return g if g < self.pairs() else -1

    def stream_of(self, g):
        return g // self.frames()

    def frame_of(self, g):
        return g % self.frames()

    def input_offset(self, g):
        return self.stream_of(g) * self.L + self.frame_of(g) * self.N

    def output_offset(self, g):
        return g * self.N

    def run_length(self, R):
        return min(max(R, 1), self.tiles())

    def runs(self, R):
        return -(-self.tiles() // self.run_length(R))

    def grid(self, max_workgroups, R):
        return min(self.runs(R), max_workgroups)

    def run_begin(self, j, R):
        return j * self.run_length(R)

    def run_end(self, j, R):
        return min((j + 1) * self.run_length(R), self.tiles())

    def schedule(self, G, R):
        """tiles of every workgroup of a grid of G, in the order the kernel visits them"""
        out = []
        for b in range(G):
            mine = []
            for j in range(b, self.runs(R), G):
                mine += range(self.run_begin(j, R), self.run_end(j, R))
            out.append(mine)
        return out


def replay(plan, G, R):
    """The kernel's loop, thread by thread (vectorised over the 256 threads and 16 registers): returns
    loads  -- list of (pair, stream, int64 array (P, N)) signal element addresses read for the pair's window (inactive slots included:
              they are marked by pair = -1 and carry the clamped pair's addresses),
    stores -- int64 array of every output element address stored, in issue order,
    taps   -- the largest coefficient index read."""
    N, P, T = plan.N, plan.P, plan.N // 16
    tid = np.arange(256)
    u, fft = tid % T, tid // T
    q = np.arange(16)
    last = plan.pairs() - 1
    loads, stores, taps = [], [], -1
    for mine in plan.schedule(G, R):
        for tile in mine:
            for j in range(plan.per_tile()):
                pair = plan.pair_of(tile, j)
                g = pair if pair >= 0 else last
                uj = u[fft == j]
                elem = (uj[:, None] + T * q[None, :]).reshape(-1)                  # the thread's sixteen elements u + T q
                addr = plan.input_offset(g) + np.arange(P, dtype=np.int64)[:, None] * N + elem[None, :]
                taps = max(taps, int((np.arange(P)[:, None] * N + elem[None, :]).max()))
                loads.append((pair, plan.stream_of(g), addr))
                if pair >= 0:
                    stores.append(plan.output_offset(g) + elem.astype(np.int64))
    return loads, (np.concatenate(stores) if stores else np.empty(0, np.int64)), taps

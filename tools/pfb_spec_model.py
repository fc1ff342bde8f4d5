"""The fp64 model of the integrated power spectra of the polyphase filter banks (include/smfft_pfb_spec.h) and of their plan
(smfft_amd/csrc/smfft_pfb_spec.hpp).

  spectra(L, N, P, T, real)     I = floor(F / T), F the bank's frames
  integrate(x, h, N, T, real)   (S, m): S[c, i, k] = sum_{t<T} p[c, i T + t, k], p the per-frame power of tools/pfb_model.py (complex
                                streams) or tools/pfb_real_model.py (real streams, packed: channel 0 is X[0]^2), and
                                m[c, i] = sum_{t<T} max_k p[c, i T + t, k], the scale of the largest-error bound
  Plan                          PfbSpecPlan, line by line (units: float2 elements, so L is the real bank's L / 2)
  replay(plan, G)               what every thread of a launch on a grid of G workgroups loads and stores

The CPU test compiles the header for the host and compares it with Plan; the GPU tests use integrate() as their reference."""
import numpy as np

import pfb_model as pm
import pfb_real_model as prm


def frames(L, N, P, real=False):
    return prm.frames(L, N, P) if real else pm.frames(L, N, P)


def spectra(L, N, P, T, real=False):
    return frames(L, N, P, real) // T


def frame_power(x, h, N, real=False):
    """(C, F, N) float64: what the bank's power mode computes per frame"""
    return prm.power(prm.pfb_real(x, h, N)) if real else pm.pfb(x, h, N, power=True)


def integrate(x, h, N, T, real=False):
    x = np.atleast_2d(np.asarray(x))
    C, L = x.shape
    P = np.asarray(h).size // ((2 if real else 1) * N)
    n = spectra(L, N, P, T, real)
    if n == 0:
        return np.empty((C, 0, N)), np.empty((C, 0))
    used = (n * T + P - 1) * (2 if real else 1) * N           # the trailing frames are not computed
    p = frame_power(x[:, :used], h, N, real)
    assert p.shape == (C, n * T, N)
    p = p.reshape(C, n, T, N)
    return p.sum(axis=2), p.max(axis=3).sum(axis=2)


class Plan:
    """smfft::PfbSpecPlan"""

    def __init__(self, L, N, P, C, T):
        self.L, self.N, self.P, self.C, self.T = L, N, P, C, T

    def frames(self):
        return pm.frames(self.L, self.N, self.P)

    def spectra(self):
        return self.frames() // self.T

    def groups(self):
        return self.spectra() * self.C

    def per_tile(self):
        return 4096 // self.N

    def tiles(self):
        return -(-self.groups() // self.per_tile())

    def group_of(self, tile, j):
        g = tile * self.per_tile() + j
        return g if g < self.groups() else -1

    def stream_of(self, g):
        return g // self.spectra()

    def spectrum_of(self, g):
        return g % self.spectra()

    def input_offset(self, g, t):
        return self.stream_of(g) * self.L + (self.spectrum_of(g) * self.T + t) * self.N

    def output_offset(self, g):
        return g * self.N

    def used(self):
        return (self.spectra() * self.T + self.P - 1) * self.N if self.spectra() else 0

    def grid(self, max_workgroups):
        return min(self.tiles(), max_workgroups)


def replay(plan, G):
    """The kernel's loop, thread by thread (vectorised over the 256 threads and 16 registers): returns
    loads  -- list of (group, stream, t, int64 array (P, N)) signal element addresses read for frame t of the group (inactive slots
              included: they are marked by group = -1 and carry the clamped group's addresses),
    stores -- int64 array of every output element address stored, in issue order,
    taps   -- the largest coefficient index read."""
    N, P, T = plan.N, plan.P, plan.N // 16
    tid = np.arange(256)
    u, fft = tid % T, tid // T
    q = np.arange(16)
    last = plan.groups() - 1
    loads, stores, taps = [], [], -1
    for b in range(G):
        for tile in range(b, plan.tiles(), G):
            for j in range(plan.per_tile()):
                group = plan.group_of(tile, j)
                g = group if group >= 0 else last
                uj = u[fft == j]
                elem = (uj[:, None] + T * q[None, :]).reshape(-1)                  # the thread's sixteen elements u + T q
                for t in range(plan.T):
                    addr = plan.input_offset(g, t) + np.arange(P, dtype=np.int64)[:, None] * N + elem[None, :]
                    loads.append((group, plan.stream_of(g), t, addr))
                taps = max(taps, int((np.arange(P)[:, None] * N + elem[None, :]).max()))
                if group >= 0:
                    stores.append(plan.output_offset(g) + elem.astype(np.int64))
    return loads, (np.concatenate(stores) if stores else np.empty(0, np.int64)), taps

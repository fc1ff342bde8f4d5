"""fp64 NumPy model of the single-pass real N = 16384 / 32768 transforms (include/smfft/smfft_large_real.hpp) + the bank conflicts of
their extra LDS exchange.

A real FFT of N = 2L points is the complex FFT of L = N/2 points (tools/large_plan_model.run replays it, thread by thread) plus a
Hermitian split (R2C, after it) or merge (C2R, before it) on the engine's layout: thread u of T = L/16 holds element k = u + T*q in
register q.  Exchange S goes through the engine's LDS image:
    write   element k at k (thread 0 also writes element 0 at L)
    read    the partner (L - k) mod L at slot L - k = (T - u) + T*(15 - q): lanes read consecutive addresses, descending
    compute a[q] = S/2 + V D, S = A + conj B, D = A - conj B (A = element k, B = its partner),
            V = -(i/2) W_N^k (R2C) or (i/2) conj W_N^k (C2R), W_N^k = W_N^u W_32^q;
            element 0: (Re A + Im A, Re A - Im A) (R2C; = (X[0], X[L])) or half of it (C2R; = (Fe[0], Fo[0]))
The packed layout is that of oracle/np_reference: element 0 = (X[0].re, X[L].re); C2R returns (N/2) x.  Conflicts are counted with the
gfx950 rules of large_plan_model.Conflicts (ds_read_b64: two 32-lane groups mod 32; ds_write_b64: four 16-lane groups mod 16).

    python tools/large_real_model.py        # prints the error against numpy.fft.rfft / c2r_packed and the conflict table
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import large_plan_model as lpm  # noqa: E402

SIZES = (16384, 32768)


def geometry(N):
    assert N in SIZES
    L = N // 2
    g = lpm.geometry(L)
    return {"N": N, "L": L, "T": g["T"], "LDS_FLOAT2": g["LDS_FLOAT2"]}


def split_rows(N, inverse):
    """V_u of every thread (u < T) and the 16 factors W_32^{+-q}, in fp64"""
    T = geometry(N)["T"]
    u = np.arange(T)
    if inverse:
        vu = 0.5j * np.exp(2j * np.pi * u / N)             # (i/2) conj W_N^u
        w32 = np.exp(2j * np.pi * np.arange(16) / 32)
    else:
        vu = -0.5j * np.exp(-2j * np.pi * u / N)           # -(i/2) W_N^u
        w32 = np.exp(-2j * np.pi * np.arange(16) / 32)
    return vu, w32


def exchange_s(regs, N, inverse, conflicts=None):
    """regs: (T, 16) complex, element u + T*q in regs[u, q] -> the split (R2C) or merge (C2R) in the same layout"""
    g = geometry(N)
    L, T = g["L"], g["T"]
    u = np.arange(T)
    lds = np.full(g["LDS_FLOAT2"], np.nan, dtype=complex)

    def waves(addr):
        return [addr[w * 64:(w + 1) * 64] for w in range(T // 64)]

    for q in range(16):
        a = u + T * q
        lds[a] = regs[:, q]
        if conflicts is not None:
            for lanes in waves(a):
                conflicts.add("S write", "w", lanes)
    lds[L] = regs[0, 0]                                    # thread 0 only: no wave-wide access
    part = np.empty_like(regs)
    for q in range(16):
        slot = (T - u) + T * (15 - q)
        assert np.array_equal(slot, L - (u + T * q))
        part[:, q] = lds[slot]
        if conflicts is not None:
            for lanes in waves(slot):
                conflicts.add("S read", "r", lanes)
    assert not np.isnan(part).any()
    vu, w32 = split_rows(N, inverse)
    A, B = regs, part
    S, D = A + np.conj(B), A - np.conj(B)
    V = vu[:, None] * w32[None, :]
    out = 0.5 * S + V * D
    a0 = regs[0, 0]
    e0 = complex(a0.real + a0.imag, a0.real - a0.imag)
    out[0, 0] = 0.5 * e0 if inverse else e0
    return out


def to_registers(z, T):
    return z[np.arange(T)[:, None] + T * np.arange(16)[None, :]]


def from_registers(regs, T):
    z = np.empty(16 * T, dtype=complex)
    z[np.arange(T)[:, None] + T * np.arange(16)[None, :]] = regs
    return z


def r2c(x, conflicts=None):
    """x: (N,) real -> (N/2,) complex packed, through the complex engine of L and the split"""
    N = x.shape[0]
    T = geometry(N)["T"]
    z = x[0::2] + 1j * x[1::2]
    Z = lpm.run(z, False)
    return from_registers(exchange_s(to_registers(Z, T), N, False, conflicts), T)


def c2r(xp, conflicts=None):
    """xp: (N/2,) complex packed -> (N,) real = (N/2) x, through the merge and the inverse complex engine of L"""
    L = xp.shape[0]
    N = 2 * L
    T = geometry(N)["T"]
    Z = from_registers(exchange_s(to_registers(np.asarray(xp, dtype=complex), T), N, True, conflicts), T)
    z = lpm.run(Z, True)
    x = np.empty(N)
    x[0::2], x[1::2] = z.real, z.imag
    return x


if __name__ == "__main__":
    from oracle import np_reference as ref
    rng = np.random.default_rng(0)
    for N in SIZES:
        x = rng.standard_normal(N)
        c = lpm.Conflicts()
        got = r2c(x, c)
        want = ref.r2c_packed(x[None])[0]
        e1 = np.linalg.norm(got - want) / np.linalg.norm(want)
        xp = rng.standard_normal(N // 2) + 1j * rng.standard_normal(N // 2)
        back = c2r(xp, c)
        want2 = ref.c2r_packed(xp[None])[0]
        e2 = np.linalg.norm(back - want2) / np.linalg.norm(want2)
        txt = "  ".join(f"{k[0]} {v:.2f}" for k, v in sorted(c.ratio().items()))
        print(f"N={N:5d} R2C relL2={e1:.1e} C2R relL2={e2:.1e}  exchange S, LDS cycles per lane group (1.00 = conflict free): {txt}")

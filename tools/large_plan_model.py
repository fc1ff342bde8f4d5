"""fp64 NumPy model of the single-pass N = 8192 / 16384 engine (include/smfft/smfft_large.hpp) + its LDS bank-conflict count.

The plan is a four-pass Stockham autosort, decimation in time, N = 16 * 16 * R * 16 with R = N / 4096, 16 elements per thread and
T = N / 16 threads per FFT.  Pass p has radix r and span Ns (the length of the sub-transforms already done):
    butterfly j reads  v[i] = x[j + i * N/r]                   (i < r)
    multiplies         v[i] *= W_{Ns*r}^{i * (j mod Ns)}
    runs               DFT_r(v)
    writes             y[(j / Ns) * Ns * r + (j mod Ns) + i * Ns] = v[i]
Passes: (r, Ns) = (16, 1), (16, 16), (R, 256), (16, N / 16).  Thread u runs butterfly u of the radix-16 passes and butterflies
u + T * b (b < 16 / R) of the radix-R pass.  The first pass reads global memory (x[u + T*i]: coalesced) and the last writes it
(y[u + T*i]); the three exchanges between go through LDS:
    A (pass 1 -> 2)  element p = 16 * a + b  at  b * SA + a,  SA = T + 2   (the only padded image: N + 32 float2)
    B (pass 2 -> 3)  element p at p
    C (pass 3 -> 4)  element p at p
The model replays every thread's registers, twiddle exponents (of the W_16384 table) and LDS addresses with the very formulas of the
header, and counts bank conflicts with the gfx950 rules of tools/plan_model.py (ds_read_b64: two 32-lane groups, bank = float2 index
mod 32; ds_write_b64: four 16-lane groups, bank = float2 index mod 16).

    python tools/large_plan_model.py        # prints error vs numpy.fft and the conflict table for both N
"""
import numpy as np

SIZES = (8192, 16384)
TABLE = 16384


def geometry(N):
    assert N in SIZES
    T = N // 16
    R = N // 4096
    SA = T + 2
    return {"N": N, "T": T, "R": R, "SA": SA, "LDS_FLOAT2": 16 * SA, "PASSES": ((16, 1), (16, 16), (R, 256), (16, N // 16))}


def lds_a(N, p):
    """physical float2 index of logical element p in exchange A"""
    g = geometry(N)
    return (p % 16) * g["SA"] + p // 16


def twiddle_exponent(N, r, Ns, i, k):
    """W_{Ns*r}^{i*k} as a power of W_16384"""
    return (i * k * (TABLE // (Ns * r))) % TABLE


class Conflicts:
    def __init__(self):
        self.acc = {}

    def add(self, name, kind, addr):
        """addr: float2 indices of one wave instruction, one per lane (64)"""
        addr = np.asarray(addr)
        assert addr.shape == (64,)
        if kind == "r":
            groups, mod = [range(0, 32), range(32, 64)], 32
        else:
            groups, mod = [range(16 * g, 16 * g + 16) for g in range(4)], 16
        cyc = 0
        for grp in groups:
            banks = addr[list(grp)] % mod
            cyc += int(np.bincount(banks, minlength=mod).max())
        c, i = self.acc.get((name, kind), (0, 0))
        self.acc[(name, kind)] = (c + cyc, i + len(groups))

    def ratio(self):
        return {k: c / i for k, (c, i) in self.acc.items()}


def dft(v, r, inverse):
    """v: (..., r) -> DFT along the last axis, un-normalised"""
    return np.fft.ifft(v, axis=-1) * r if inverse else np.fft.fft(v, axis=-1)


def run(x, inverse=False, conflicts=None):
    """x: (N,) complex -> the plan's result, replayed thread by thread (vectorised over threads)"""
    N = x.shape[0]
    g = geometry(N)
    T, R = g["T"], g["R"]
    u = np.arange(T)
    tw = np.exp((2j if inverse else -2j) * np.pi * np.arange(TABLE) / TABLE)
    lds = np.full(g["LDS_FLOAT2"], np.nan, dtype=complex)

    def wave_lanes(addr_per_thread):
        return [addr_per_thread[w * 64:(w + 1) * 64] for w in range(T // 64)]

    # pass 1: r[c] = x[u + T*c], DFT_16
    regs = x[u[:, None] + T * np.arange(16)[None, :]]
    regs = dft(regs, 16, inverse)
    # exchange A: element p = 16*u + i at (p % 16) * SA + p // 16 = i * SA + u
    for i in range(16):
        a = lds_a(N, 16 * u + i)
        assert np.array_equal(a, i * g["SA"] + u)
        lds[a] = regs[:, i]
        if conflicts is not None:
            for lanes in wave_lanes(a):
                conflicts.add("A write", "w", lanes)
    # pass 2: read p = u + T*i, twiddle W_256^{i*(u % 16)}
    regs = np.empty((T, 16), dtype=complex)
    for i in range(16):
        p = u + T * i
        a = lds_a(N, p)
        regs[:, i] = lds[a]
        if conflicts is not None:
            for lanes in wave_lanes(a):
                conflicts.add("A read", "r", lanes)
    k = u % 16
    for i in range(1, 16):
        regs[:, i] *= tw[twiddle_exponent(N, 16, 16, i, k)]
    regs = dft(regs, 16, inverse)
    lds[:] = np.nan
    for i in range(16):
        p = (u // 16) * 256 + u % 16 + 16 * i
        lds[p] = regs[:, i]
        if conflicts is not None:
            for lanes in wave_lanes(p):
                conflicts.add("B write", "w", lanes)
    # pass 3: B = 16 / R butterflies per thread, j = u + T*b, reads p = j + (N/R)*i, twiddle W_{256R}^{i*(j % 256)}
    B = 16 // R
    out3 = {}
    for b in range(B):
        j = u + T * b
        v = np.empty((T, R), dtype=complex)
        for i in range(R):
            p = j + (N // R) * i
            v[:, i] = lds[p]
            if conflicts is not None:
                for lanes in wave_lanes(p):
                    conflicts.add("B read", "r", lanes)
        for i in range(1, R):
            v[:, i] *= tw[twiddle_exponent(N, R, 256, i, j % 256)]
        out3[b] = (j, dft(v, R, inverse))
    lds[:] = np.nan
    for b in range(B):
        j, v = out3[b]
        for i in range(R):
            p = (j // 256) * 256 * R + j % 256 + 256 * i
            lds[p] = v[:, i]
            if conflicts is not None:
                for lanes in wave_lanes(p):
                    conflicts.add("C write", "w", lanes)
    # pass 4: read p = u + T*i, twiddle W_N^{i*u}, DFT_16, y[u + T*i]
    regs = np.empty((T, 16), dtype=complex)
    for i in range(16):
        p = u + T * i
        regs[:, i] = lds[p]
        if conflicts is not None:
            for lanes in wave_lanes(p):
                conflicts.add("C read", "r", lanes)
    for i in range(1, 16):
        regs[:, i] *= tw[twiddle_exponent(N, 16, N // 16, i, u)]
    regs = dft(regs, 16, inverse)
    y = np.empty(N, dtype=complex)
    y[u[:, None] + T * np.arange(16)[None, :]] = regs
    return y


def twiddle_rows(N):
    """The exponents (powers of W_16384) of the per-N twiddle rows the header builds at compile time:
    w2[(i-1)*16 + k] = W_256^{i*k}, w3[(i-1)*256 + k] = W_{256R}^{i*k}, w4[(i-1)*T + u] = W_N^{i*u}."""
    g = geometry(N)
    T, R = g["T"], g["R"]
    w2 = [twiddle_exponent(N, 16, 16, i, k) for i in range(1, 16) for k in range(16)]
    w3 = [twiddle_exponent(N, R, 256, i, k) for i in range(1, R) for k in range(256)]
    w4 = [twiddle_exponent(N, 16, N // 16, i, u) for i in range(1, 16) for u in range(T)]
    return w2, w3, w4


if __name__ == "__main__":
    rng = np.random.default_rng(0)
    for N in SIZES:
        x = rng.standard_normal(N) + 1j * rng.standard_normal(N)
        for inv in (False, True):
            c = Conflicts()
            y = run(x, inv, c)
            want = np.fft.ifft(x) * N if inv else np.fft.fft(x)
            err = np.linalg.norm(y - want) / np.linalg.norm(want)
            txt = "  ".join(f"{k[0]} {v:.2f}" for k, v in sorted(c.ratio().items()))
            print(f"N={N:5d} inverse={int(inv)} relL2={err:.1e}  LDS cycles per lane group (1.00 = conflict free): {txt}")

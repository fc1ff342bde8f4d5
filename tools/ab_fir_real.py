"""The overlap-save filter bank for real signals and real taps (smfft_fir_real_benchmark) against what a user of real data had before it,
on ONE signal in ONE process, timed round robin so that drift of the box hits all alike:
  real bank:            smfft_fir_real_benchmark on the float32 signal -- the shipped build and every build given with --alt (the other
                        form of the signal loads: make -C smfft_amd/csrc FIR_REAL_NT_LOADS=0 FIR_REAL_LIB=... FIR_REAL_OBJDIR=...)
  complex bank:         smfft_fir_benchmark on the complex64 cast of the same signal, the cast made beforehand
  cast + complex bank:  the cast itself (torch, on the device) and then smfft_fir_launch, between two events
  copy:                 a device copy that moves the real bank's input and output bytes, (C L + C K L) * 4: the same-run ceiling
Shapes: the headline FIR shape C = 1, L = 2^24, K = 32, M = 257 at N = 1024 and at N = 2048 -- the real bank's overlap efficiency is
(N - M + 1) / N per REAL segment, so where a user would pick the next N is a result of this run, not an assumption.  Every entry is
warmed up twice; medians, quartiles and minima over --reps rounds, which run through the entries forwards and backwards in turn (what ran just
before an entry changes with the direction, so two builds of one kernel are not timed in one fixed order).  Before the timing the real bank's output is compared with the real part of the complex bank's (and the builds with each other, to the bit).  RATIO lines: real / complex, real / (cast + complex),
real / copy per N, and the best N of each bank.
    python tools/ab_fir_real.py [--reps 30] [--alt NAME=lib.so ...] [--small] > profiles/r16_fir_real_ab.txt"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import smfft_amd as sm  # noqa: E402
from smfft_amd import fir_real  # noqa: E402
from ab_fir_common import round_robin  # noqa: E402  (beside this file)
from ab_fir_common import timed as events  # noqa: E402

COPY = "copy of the real bank's bytes"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--alt", action="append", default=[], metavar="NAME=PATH", help="another build of libsmfft_fir_real.so")
    ap.add_argument("--small", action="store_true", help="a sixteenth of the signal (a rehearsal, not a measurement)")
    args = ap.parse_args()
    sm.FFT_init()
    torch.cuda.init()
    stream = torch.cuda.current_stream()          # the default stream: the *_benchmark entry points time on the null stream
    sp = stream.cuda_stream
    builds = {"shipped": fir_real.lib()}
    for item in args.alt:
        name, path = item.split("=", 1)
        builds[name] = fir_real.load(os.path.abspath(path))
    print(f"device: {torch.cuda.get_device_name(0)}; {args.reps} reps round robin; builds of libsmfft_fir_real.so: {', '.join(builds)}", flush=True)

    C, L, K, M = 1, (1 << 24) // (16 if args.small else 1), 32, 257
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.empty((C, L), dtype=torch.float32, device="cuda").normal_(generator=gen)
    h = torch.empty((K, M), dtype=torch.float32, device="cuda").normal_(generator=gen) / 16
    xc, hc = x.to(torch.complex64), h.to(torch.complex64)
    out_r = torch.empty((C, K, L), dtype=torch.float32, device="cuda")
    out_c = torch.empty((C, K, L), dtype=torch.complex64, device="cuda")
    cast = torch.empty_like(xc)
    moved = (C * L + C * K * L) * 4
    src = torch.empty(moved // 8, dtype=torch.float32, device="cuda").normal_(generator=gen)
    dst = torch.empty_like(src)
    medians = {}
    for N in (1024, 2048):
        V = N - M + 1
        S = -(-L // V)
        Hr = torch.empty((K, N), dtype=torch.complex64, device="cuda")
        Hc = torch.empty_like(Hr)
        fir_real.prepare(h.data_ptr(), Hr.data_ptr(), M, K, N, "convolve", stream=sp)
        sm.fir_prepare(hc.data_ptr(), Hc.data_ptr(), M, K, N, "convolve", stream=sp)
        torch.cuda.synchronize()
        print(f"--- C={C} L={L} K={K} M={M} N={N}: V={V}, {S} segments = {(S + 1) // 2} pairs; real bank {moved / 2**30:.2f} GiB moved, "
              f"complex bank {2 * moved / 2**30:.2f} GiB", flush=True)

        def real(lib):
            def run():
                t = ctypes.c_double(0.0)
                rc = lib.smfft_fir_real_benchmark(x.data_ptr(), L, C, Hr.data_ptr(), K, M, N, 0, out_r.data_ptr(), ctypes.byref(t))
                assert rc == 0, rc
                return t.value
            return run

        def cplx():
            t = ctypes.c_double(0.0)
            rc = sm.lib.smfft_fir_benchmark(xc.data_ptr(), L, C, Hc.data_ptr(), K, M, N, 0, out_c.data_ptr(), ctypes.byref(t))
            assert rc == 0, rc
            return t.value

        def cast_and_cplx():
            def run():
                cast.copy_(x)
                sm.fir_launch(cast.data_ptr(), L, C, Hc.data_ptr(), K, M, N, out_c.data_ptr(), "convolve", stream=sp)
            return events(run, stream)

        # the same results first: the builds to the bit, the real bank against the real part of the complex bank
        base = None
        for name, lib in builds.items():
            out_r.fill_(float("nan"))
            real(lib)()
            if base is None:
                base = out_r.clone()
            else:
                assert torch.equal(out_r.view(torch.int32), base.view(torch.int32)), f"{name}: bits differ from the shipped build"
        out_c.fill_(0)
        cplx()
        torch.cuda.synchronize()
        scale = out_c.real.abs().max().item()
        print(f"max |real bank - Re(complex bank)| / max = {(base - out_c.real).abs().max().item() / scale:.2e}; "
              f"max |Im(complex bank)| / max = {out_c.imag.abs().max().item() / scale:.2e} (the half the cast user throws away)", flush=True)
        n0, W = L - 5000, 5000
        want = np.convolve(x[0, n0 - (M - 1):].cpu().numpy().astype(np.float64), h[K - 1].cpu().numpy().astype(np.float64))[M - 1:M - 1 + W]
        got = base[0, K - 1, n0:].cpu().numpy()
        print(f"real bank vs np.convolve (last row, last {W}): relL2 {np.linalg.norm(got - want) / np.linalg.norm(want):.2e}", flush=True)
        del base

        fns = {f"real bank ({name})": real(lib) for name, lib in builds.items()}
        fns["complex bank on the cast signal"] = cplx
        fns["cast + complex bank"] = cast_and_cplx
        fns[COPY] = lambda: events(lambda: dst.copy_(src), stream)
        ts = round_robin(fns, args.reps, alternate=True)      # every fn returns its own milliseconds
        q = {n: (v[len(v) // 4], v[len(v) // 2], v[(3 * len(v)) // 4]) for n, v in ts.items()}
        for n, v in ts.items():
            lo, med, hi = q[n]
            nbytes = moved if n.startswith("real") or n == COPY else 2 * moved + (C * L * 12 if n.startswith("cast") else 0)
            print(f"{n:34s} median {med:8.3f} ms  quartiles {lo:8.3f} {hi:8.3f}  min {v[0]:8.3f}  {nbytes / med / 1e9:6.3f} TB/s of its own bytes", flush=True)
        r = q["real bank (shipped)"][1]
        print(f"RATIO N={N}: real / complex = {r / q['complex bank on the cast signal'][1]:.4f}, real / (cast + complex) = "
              f"{r / q['cast + complex bank'][1]:.4f}, real / copy = {r / q[COPY][1]:.4f}", flush=True)
        for name in builds:
            if name != "shipped":
                print(f"BUILDS N={N}: shipped {r:.4f} ms, {name} {q[f'real bank ({name})'][1]:.4f} ms, shipped / {name} = {r / q[f'real bank ({name})'][1]:.4f}", flush=True)
        medians[N] = (r, q["complex bank on the cast signal"][1])
        del Hr, Hc
    best_r, best_c = min(medians, key=lambda n: medians[n][0]), min(medians, key=lambda n: medians[n][1])
    print(f"RATIO best N: real bank N={best_r} {medians[best_r][0]:.3f} ms, complex bank N={best_c} {medians[best_c][1]:.3f} ms, "
          f"real / complex = {medians[best_r][0] / medians[best_c][1]:.4f}", flush=True)


if __name__ == "__main__":
    main()

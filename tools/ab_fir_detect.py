"""The detected filter banks (smfft_fir_power_benchmark, smfft_fir_peak_benchmark) against what a caller had before them, on ONE signal in
ONE process, timed round robin so that drift of the box hits all alike:
  power (fused):        smfft_fir_power_benchmark -- the shipped build and every build given with --alt
  peak (fused):         smfft_fir_peak_benchmark -- the same builds (another home of the peak kernel's winners: make -C smfft_amd/csrc
                        FIR_DETECT_WINNERS=1 FIR_DETECT_LIB=... FIR_DETECT_OBJDIR=...; 0 registers, 1 LDS, 2 index in LDS, 3 registers
                        without the spectrum prefetch)
  bank + power:         smfft_fir_benchmark into the C K L complex buffer, plus torch real^2 + imag^2 into a float buffer, between events
  bank + power + max:   the same plus torch.max over the filters (values and indices)
Shapes: the headline FIR shape C = 1, L = 2^24, K = 32, M = 257 at N = 1024 and at N = 2048.  Every entry is warmed up twice; medians,
quartiles and minima over --reps rounds, which run through the entries forwards and backwards in turn.  Before the timing the fused
outputs are compared with the pipeline's (the power to the bit where torch rounds alike, else by its largest relative difference; the
peak against the maximum of the fused power to the bit) and the builds with each other, to the bit.  Per entry: the fraction of the HBM
floor of its own bytes at 8 TB/s and the fp32 fraction by the formula of DESIGN.md section 2.3b (5 N log2 N flop per transform; forward
transforms x filter groups + inverse transforms; one filter group in the peak launch).  RATIO lines: fused / pipeline per N, and the
workspace the fused launches do without.
    python tools/ab_fir_detect.py [--reps 30] [--alt NAME=lib.so ...] [--small] > profiles/r17_fir_detect_ab.txt"""
import argparse
import ctypes
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import smfft_amd as sm  # noqa: E402
from smfft_amd import fir_detect  # noqa: E402
from ab_fir_common import round_robin  # noqa: E402  (beside this file)
from ab_fir_common import timed as events  # noqa: E402

FP32_PEAK_TFLOPS = 157.3     # bench.py
HBM_TBS = 8.0
TARGET_WORKGROUPS = 2048     # smfft_fir_kernel.hpp, kFirTargetWorkgroups


def groups_of(tiles, K):
    g = min(K, max(1, -(-TARGET_WORKGROUPS // tiles)))
    return -(-K // -(-K // g))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--alt", action="append", default=[], metavar="NAME=PATH", help="another build of libsmfft_fir_detect.so")
    ap.add_argument("--small", action="store_true", help="a sixteenth of the signal (a rehearsal, not a measurement)")
    args = ap.parse_args()
    sm.FFT_init()
    torch.cuda.init()
    stream = torch.cuda.current_stream()          # the default stream: the *_benchmark entry points time on the null stream
    sp = stream.cuda_stream
    builds = {"shipped": fir_detect.lib()}
    for item in args.alt:
        name, path = item.split("=", 1)
        builds[name] = fir_detect.load(os.path.abspath(path))
    print(f"device: {torch.cuda.get_device_name(0)}; {args.reps} reps round robin; builds of libsmfft_fir_detect.so: {', '.join(builds)}", flush=True)

    C, L, K, M = 1, (1 << 24) // (16 if args.small else 1), 32, 257
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.view_as_complex(torch.empty((C, L, 2), dtype=torch.float32, device="cuda").normal_(generator=gen))
    h = torch.view_as_complex(torch.empty((K, M, 2), dtype=torch.float32, device="cuda").normal_(generator=gen) / 16)
    y = torch.empty((C, K, L), dtype=torch.complex64, device="cuda")            # the pipeline's workspace
    p_pipe = torch.empty((C, K, L), dtype=torch.float32, device="cuda")
    tmp = torch.empty((C, K, L), dtype=torch.float32, device="cuda")            # (torch's imag^2 before the sum)
    best_pipe = torch.empty((C, L), dtype=torch.float32, device="cuda")
    arg_pipe = torch.empty((C, L), dtype=torch.int64, device="cuda")
    p_fused = torch.empty((C, K, L), dtype=torch.float32, device="cuda")
    best = torch.empty((C, L), dtype=torch.float32, device="cuda")
    index = torch.empty((C, L), dtype=torch.int32, device="cuda")
    in_bytes = C * L * 8
    own = {"power": in_bytes + C * K * L * 4, "peak": in_bytes + C * L * 8,
           # the bank's 8 B per element out; re^2 and im^2 each read the complex rows' cache lines (8 B) and write 4 B; the sum reads two
           # floats and writes one; the maximum reads the powers and writes a float and an int64 per sample
           "bank + power": in_bytes + C * K * L * (8 + 12 + 12 + 12), "bank + power + max": in_bytes + C * K * L * (8 + 12 + 12 + 12 + 4) + C * L * 12}
    print(f"workspace: the pipeline holds C K L complex64 = {C * K * L * 8 / 2**30:.2f} GiB (+ {C * K * L * 4 / 2**30:.2f} GiB of powers before "
          f"the maximum); the fused power launch holds only its {C * K * L * 4 / 2**30:.2f} GiB output, the fused peak launch {C * L * 8 / 2**20:.0f} MiB", flush=True)
    for N in (1024, 2048):
        V = N - M + 1
        S = -(-L // V)
        tiles = -(-(C * S) // (4096 // N))
        H = torch.empty((K, N), dtype=torch.complex64, device="cuda")
        sm.fir_prepare(h.data_ptr(), H.data_ptr(), M, K, N, "convolve", stream=sp)
        torch.cuda.synchronize()
        flop = {"power": C * S * (groups_of(tiles, K) + K), "peak": C * S * (1 + K)}
        flop = {k: v * 5 * N * math.log2(N) for k, v in flop.items()}
        flop["bank + power"] = flop["bank + power + max"] = flop["power"]
        print(f"--- C={C} L={L} K={K} M={M} N={N}: V={V}, {S} segments, {tiles} tiles, {groups_of(tiles, K)} filter group(s) in the power launch", flush=True)

        def fused(lib, what):
            def run():
                t = ctypes.c_double(0.0)
                if what == "power":
                    rc = lib.smfft_fir_power_benchmark(x.data_ptr(), L, C, H.data_ptr(), K, M, N, 0, p_fused.data_ptr(), ctypes.byref(t))
                else:
                    rc = lib.smfft_fir_peak_benchmark(x.data_ptr(), L, C, H.data_ptr(), K, M, N, 0, best.data_ptr(), index.data_ptr(), ctypes.byref(t))
                assert rc == 0, rc
                return t.value
            return run

        def pipeline(with_max):
            def run():
                sm.fir_launch(x.data_ptr(), L, C, H.data_ptr(), K, M, N, y.data_ptr(), "convolve", stream=sp)
                yr = torch.view_as_real(y)
                torch.mul(yr[..., 0], yr[..., 0], out=p_pipe)
                torch.mul(yr[..., 1], yr[..., 1], out=tmp)
                p_pipe.add_(tmp)
                if with_max:
                    torch.max(p_pipe, dim=1, out=(best_pipe, arg_pipe))
            return lambda: events(run, stream)

        # the same results first
        base = None
        for name, lib in builds.items():
            p_fused.fill_(float("nan")), best.fill_(float("nan")), index.fill_(-1)
            fused(lib, "power")(), fused(lib, "peak")()
            now = (p_fused.clone(), best.clone(), index.clone())
            assert torch.equal(now[1].view(torch.int32), now[0].max(dim=1).values.view(torch.int32)), f"{name}: peak is not the maximum of the power rows"
            assert torch.equal(now[2].long(), now[0].max(dim=1).indices) or torch.equal(now[0].gather(1, now[2].long()[:, None])[:, 0], now[1]), name
            assert int(now[2].min()) >= 0 and int(now[2].max()) < K
            if base is None:
                base = now
            else:
                assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(now, base)), f"{name}: bits differ from the shipped build"
        pipeline(True)()
        torch.cuda.synchronize()
        scale = p_pipe.max().item()
        print(f"max |fused power - pipeline power| / max = {(base[0] - p_pipe).abs().max().item() / scale:.2e}; "
              f"max |fused peak - pipeline peak| / max = {(base[1] - best_pipe).abs().max().item() / scale:.2e}; "
              f"indices that differ from the pipeline's: {int((base[2].long() != arg_pipe).sum())} of {C * L}", flush=True)
        n0, W = L - 5000, 5000
        want = np.convolve(x[0, n0 - (M - 1):].cpu().numpy().astype(np.complex128), h[K - 1].cpu().numpy().astype(np.complex128))[M - 1:M - 1 + W]
        got = base[0][0, K - 1, n0:].cpu().numpy()
        print(f"fused power vs |np.convolve|^2 (last row, last {W}): max rel {np.max(np.abs(got - np.abs(want) ** 2)) / np.max(np.abs(want) ** 2):.2e}", flush=True)
        del base, now

        fns = {}
        for name, lib in builds.items():
            fns[f"power ({name})"] = fused(lib, "power")
            fns[f"peak ({name})"] = fused(lib, "peak")
        fns["bank + power"] = pipeline(False)
        fns["bank + power + max"] = pipeline(True)
        ts = round_robin(fns, args.reps, alternate=True)      # every fn returns its own milliseconds
        q = {n: (v[len(v) // 4], v[len(v) // 2], v[(3 * len(v)) // 4]) for n, v in ts.items()}
        for n, v in ts.items():
            lo, med, hi = q[n]
            kind = n.split(" (")[0]
            floor = own[kind] / (HBM_TBS * 1e12) * 1e3
            frac = flop[kind] / (med * 1e-3) / 1e12 / FP32_PEAK_TFLOPS
            print(f"{n:28s} median {med:8.3f} ms  quartiles {lo:8.3f} {hi:8.3f}  min {v[0]:8.3f}  HBM floor of its own bytes {floor:6.3f} ms "
                  f"({floor / med:.2f} of it)  {frac:.3f} of fp32 peak", flush=True)
        pw, pk = q["power (shipped)"], q["peak (shipped)"]
        a, b = q["bank + power"], q["bank + power + max"]
        print(f"RATIO N={N}: power / (bank + power) = {pw[1] / a[1]:.4f} (quartiles {pw[0] / a[2]:.4f} ... {pw[2] / a[0]:.4f}), "
              f"peak / (bank + power + max) = {pk[1] / b[1]:.4f} (quartiles {pk[0] / b[2]:.4f} ... {pk[2] / b[0]:.4f})", flush=True)
        for name in builds:
            if name != "shipped":
                print(f"BUILDS N={N}: peak shipped {pk[1]:.4f} ms, {name} {q[f'peak ({name})'][1]:.4f} ms, shipped / {name} = {pk[1] / q[f'peak ({name})'][1]:.4f}; "
                      f"power shipped {pw[1]:.4f} ms, {name} {q[f'power ({name})'][1]:.4f} ms", flush=True)
        del H


if __name__ == "__main__":
    main()

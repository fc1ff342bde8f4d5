"""The DCT / DST kernels (smfft_dct_benchmark) against their other builds and against what a caller had before them, on ONE pair of
buffers in ONE process, timed round robin so that drift of the box hits all alike:
  dct:     smfft_dct_benchmark, one fused launch (the library's own events) -- the shipped build and every build given with
           --alt NAME=PATH: the row accesses as 4-byte accesses at stride four instead of 16-byte accesses and a pass through LDS
           (make -C smfft_amd/csrc DCT_STAGED=0 DCT_LIB=... DCT_OBJDIR=... <that DCT_LIB>), plain instead of non-temporal 16-byte
           accesses (EXTRA_HIPFLAGS=-DSMFFT_NT=0) and non-temporal instead of plain 4-byte accesses
           (EXTRA_HIPFLAGS="-DSMFFT_DCT_NT_LOAD1=1 -DSMFFT_DCT_NT_STORE1=1").  All builds must give the same bits
  torch:   the unfused pipeline on the same buffers between events.  Type II: the index permutation v = x[perm], torch.fft.fft of v,
           the quarter-wave twiddle product, twice the real part copied out.  Type III: the twiddle product of X[k] - i X[n - k], the
           un-normalised inverse fft, the real part gathered back through the inverse permutation
  copy:    a copy_ of the same bytes (n floats in, n floats out per row), between events
Shapes: 2 GiB of float32 input (2^29 elements) as rows of n = 512, 2048 and 8192 (--lengths: others); types II and III of the cosine transform (the sine
transforms are the same kernels with other index arithmetic).  Every entry is warmed up twice; medians, quartiles and minima over
--reps rounds, which run through the entries forwards and backwards in turn (the method of DESIGN.md section 21).  Before the timing
the output is compared with the pipeline's and a sample of rows with the fp64 chain of tools/dct_model.py, and the builds with the
shipped one to the bit.  RATIO lines: dct / torch, dct / copy; BUILDS lines: shipped / other.
    python tools/ab_dct.py [--reps 15] [--lengths 512 1024 2048 4096 8192] [--alt NAME=lib.so ...] [--small] > profiles/r22_dct_ab.txt"""
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
from smfft_amd import dct  # noqa: E402
import dct_model as dm  # noqa: E402  (beside this file)
from ab_fir_common import round_robin  # noqa: E402
from ab_fir_common import timed as events  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--alt", action="append", default=[], metavar="NAME=PATH", help="another build of libsmfft_dct.so")
    ap.add_argument("--lengths", type=int, nargs="+", default=[512, 2048, 8192], help="the row lengths n")
    ap.add_argument("--small", action="store_true", help="a sixty-fourth of the buffers (a rehearsal, not a measurement)")
    args = ap.parse_args()
    sm.FFT_init()
    torch.cuda.init()
    stream = torch.cuda.current_stream()          # the default stream: the benchmark entry point times on the null stream
    builds = {"shipped": dct.lib()}
    for item in args.alt:
        name, path = item.split("=", 1)
        builds[name] = dct.load(os.path.abspath(path))
    elements = (1 << 29) // (64 if args.small else 1)
    print(f"device: {torch.cuda.get_device_name(0)}; {args.reps} reps round robin; {elements * 4 / 2**30:.3f} GiB of input; "
          f"builds of libsmfft_dct.so: {', '.join(builds)}", flush=True)
    gen = torch.Generator(device="cuda").manual_seed(0)
    x_all = torch.empty(elements, dtype=torch.float32, device="cuda").normal_(generator=gen)
    y_all = torch.empty(elements, dtype=torch.float32, device="cuda")
    y_ref = torch.empty(elements, dtype=torch.float32, device="cuda")
    spare = torch.empty(elements, dtype=torch.float32, device="cuda")
    same_bits = True
    for n in args.lengths:
        batch = elements // n
        M = n // 2
        x, y, yr = x_all.view(batch, n), y_all.view(batch, n), y_ref.view(batch, n)
        moved = 2 * batch * n * 4
        j = torch.arange(n, device="cuda")
        perm = torch.where(j < M, 2 * j, 2 * (n - 1 - j) + 1)              # v[j] = x[perm[j]]
        inverse = torch.empty_like(perm)
        inverse[perm] = j
        ang = -math.pi * torch.arange(n, device="cuda", dtype=torch.float64) / (2 * n)
        w = torch.polar(torch.ones_like(ang), ang).to(torch.complex64)     # W_4n^k, k < n
        for type in (2, 3):
            print(f"--- DCT-{'II' if type == 2 else 'III'} n={n} M={M} batch={batch}: {-(-batch // (4096 // M))} tiles, {moved / 2**30:.2f} GiB moved (in + out, float32)", flush=True)

            def fused(lib):
                def run():
                    t = ctypes.c_double(0.0)
                    rc = lib.smfft_dct_benchmark(x.data_ptr(), y.data_ptr(), n, batch, type, 0, ctypes.byref(t))
                    assert rc == 0, rc
                    return t.value
                return run

            def pipeline():
                if type == 2:
                    spectrum = torch.fft.fft(x[:, perm], dim=-1)
                    spectrum *= w
                    torch.mul(spectrum.real, 2.0, out=yr)
                else:
                    mirrored = torch.cat([torch.zeros_like(x[:, :1]), x.flip(-1)[:, :-1]], dim=-1)       # X[n - k], X[n] := 0
                    spectrum = torch.complex(x, -mirrored)
                    spectrum *= w.conj()
                    yr.copy_(torch.fft.ifft(spectrum, dim=-1, norm="forward").real[:, inverse])

            # the same results first
            base = None
            for name, lib in builds.items():
                y.fill_(float("nan"))
                fused(lib)()
                if base is None:
                    base = y.clone()
                else:
                    differ = int((y.view(torch.int32) != base.view(torch.int32)).sum().item())
                    print(f"{name}: {differ} of {y.numel()} outputs differ from the shipped build's bits"
                          + (f", max |d| / max = {(y - base).abs().max().item() / base.abs().max().item():.2e}" if differ else ""), flush=True)
                    same_bits = same_bits and differ == 0
            del base
            events(pipeline, stream)
            torch.cuda.synchronize()
            print(f"max |dct - torch| / max = {(y - yr).abs().max().item() / yr.abs().max().item():.2e}", flush=True)
            rows = [0, batch // 2, batch - 1]
            want = dm.chain(x[rows].cpu().numpy(), type, False)
            for name, out in (("dct", y), ("torch", yr)):
                l2, mx = dm.errors(out[rows].cpu().numpy(), want)
                print(f"{name} vs the fp64 chain (rows {rows}): worst row relL2 {l2:.2e}, max |d| / max |want| {mx:.2e}", flush=True)

            fns = {("dct" if name == "shipped" else f"dct ({name})"): fused(lib) for name, lib in builds.items()}
            fns.update({"torch": lambda: events(pipeline, stream), "copy": lambda: events(lambda: spare.copy_(x_all), stream)})
            ts = round_robin(fns, args.reps, alternate=True)      # every fn returns its own milliseconds
            q = {k: (v[len(v) // 4], v[len(v) // 2], v[(3 * len(v)) // 4]) for k, v in ts.items()}
            for k, v in ts.items():
                lo, med, hi = q[k]
                print(f"{k:24s} median {med:8.3f} ms  quartiles {lo:8.3f} {hi:8.3f}  min {v[0]:8.3f}  {moved / (med * 1e-3) / 1e12:6.3f} TB/s (the launch's bytes)  "
                      f"{med / q['copy'][1]:6.3f} x the copy", flush=True)
            c = q["dct"]
            what = f"DCT-{'II' if type == 2 else 'III'} n={n}"
            print(f"RATIO {what}: " + ", ".join(f"dct / {k} = {c[1] / o[1]:.4f} (quartiles {c[0] / o[2]:.4f} ... {c[2] / o[0]:.4f})"
                                                for k, o in ((k, q[k]) for k in ("torch", "copy"))), flush=True)
            for name in builds:
                if name != "shipped":
                    alt = q[f"dct ({name})"]
                    sep = "separate" if c[2] < alt[0] or alt[2] < c[0] else "overlap: tie"
                    print(f"BUILDS {what}: shipped {c[1]:.4f} ms (quartiles {c[0]:.4f} ... {c[2]:.4f}), {name} {alt[1]:.4f} ms (quartiles {alt[0]:.4f} ... {alt[2]:.4f}), "
                          f"shipped / {name} = {c[1] / alt[1]:.4f}; quartile ranges {sep}", flush=True)
        torch.cuda.empty_cache()
    assert same_bits, "a build's bits differ from the shipped build's (see above)"


if __name__ == "__main__":
    main()

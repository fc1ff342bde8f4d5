"""The arbitrary-length FFTs (smfft_bluestein_benchmark) against what a caller had before them, on ONE buffer in ONE process, timed round
robin so that drift of the box hits all alike:
  bluestein:   smfft_bluestein_benchmark, one fused launch (the library's own events) -- the shipped build and every build given with
               --alt (plain instead of non-temporal row loads and stores: make -C smfft_amd/csrc EXTRA_HIPFLAGS=-DSMFFT_NT=0
               BLUESTEIN_LIB=... BLUESTEIN_OBJDIR=... <that BLUESTEIN_LIB>)
  torch.fft:   torch.fft.fft(x, out=y) on the same buffer viewed as (batch, n), between events (hipFFT behind it)
  copy:        y.copy_(x) of the same bytes, between events: the ceiling of anything that reads and writes every byte once
Shapes: 4 GiB of complex64 in (2^29 elements; batch = 2^29 // n rows) at n = 1000, 1536, 2039, and 1024 for reference (a power of
two, which smfft_launch serves more cheaply).  Every entry is warmed up twice; medians, quartiles and minima over --reps rounds, which
run through the entries forwards and backwards in turn.  Before the timing the fused output is compared with torch.fft's and a sample
of rows with fp64 np.fft.  Per entry: the bytes it moves per second (in + out) and its time over the same-run copy's.  RATIO lines:
bluestein / torch.fft and bluestein / copy per n; BUILDS lines: shipped / other build.
    python tools/ab_bluestein.py [--reps 20] [--alt NAME=lib.so ...] [--small] > profiles/r18_bluestein_ab.txt"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import smfft_amd as sm  # noqa: E402
from smfft_amd import bluestein  # noqa: E402
from ab_fir_common import round_robin  # noqa: E402  (beside this file)
from ab_fir_common import timed as events  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--alt", action="append", default=[], metavar="NAME=PATH", help="another build of libsmfft_bluestein.so")
    ap.add_argument("--small", action="store_true", help="a sixty-fourth of the buffer (a rehearsal, not a measurement)")
    args = ap.parse_args()
    sm.FFT_init()
    torch.cuda.init()
    stream = torch.cuda.current_stream()          # the default stream: smfft_bluestein_benchmark times on the null stream
    builds = {"shipped": bluestein.lib()}
    for item in args.alt:
        name, path = item.split("=", 1)
        builds[name] = bluestein.load(os.path.abspath(path))
    elements = (1 << 29) // (64 if args.small else 1)
    print(f"device: {torch.cuda.get_device_name(0)}; {args.reps} reps round robin; {elements * 8 / 2**30:.3f} GiB in, as much out; "
          f"builds of libsmfft_bluestein.so: {', '.join(builds)}", flush=True)
    gen = torch.Generator(device="cuda").manual_seed(0)
    x_all = torch.view_as_complex(torch.empty((elements, 2), dtype=torch.float32, device="cuda").normal_(generator=gen))
    y_all = torch.empty(elements, dtype=torch.complex64, device="cuda")
    y_ref = torch.empty(elements, dtype=torch.complex64, device="cuda")
    for n in (1000, 1536, 2039, 1024):
        batch = elements // n
        M = bluestein.fft_size(n)
        x, y, yr = (t[:batch * n].view(batch, n) for t in (x_all, y_all, y_ref))
        plan = torch.empty(2 * M, dtype=torch.complex64, device="cuda")
        bluestein.prepare(n, plan.data_ptr())
        moved = 2 * batch * n * 8
        print(f"--- n={n} M={M} batch={batch}: {-(-batch // (4096 // M))} tiles, {moved / 2**30:.2f} GiB moved (in + out)", flush=True)

        def fused(lib):
            def run():
                t = ctypes.c_double(0.0)
                rc = lib.smfft_bluestein_benchmark(x.data_ptr(), y.data_ptr(), n, batch, plan.data_ptr(), ctypes.byref(t))
                assert rc == 0, rc
                return t.value
            return run

        def vendor():
            return events(lambda: torch.fft.fft(x, dim=-1, out=yr), stream)

        def copy():
            return events(lambda: yr.copy_(x), stream)

        # the same results first
        base = None
        for name, lib in builds.items():
            y.fill_(float("nan"))
            fused(lib)()
            if base is None:
                base = y.clone()
            else:
                assert torch.equal(y.view(torch.int64), base.view(torch.int64)), f"{name}: bits differ from the shipped build"
        del base
        vendor()
        torch.cuda.synchronize()
        scale = yr.abs().max().item()
        print(f"max |bluestein - torch.fft| / max |torch.fft| = {(y - yr).abs().max().item() / scale:.2e}", flush=True)
        rows = [0, batch // 2, batch - 1]
        want = np.fft.fft(x[rows].cpu().numpy().astype(np.complex128), axis=-1)
        for name, out in (("bluestein", y), ("torch.fft", yr)):
            d = out[rows].cpu().numpy().astype(np.complex128) - want
            print(f"{name} vs fp64 np.fft (rows {rows}): worst relL2 {np.max(np.linalg.norm(d, axis=1) / np.linalg.norm(want, axis=1)):.2e}", flush=True)

        fns = {("bluestein" if name == "shipped" else f"bluestein ({name})"): fused(lib) for name, lib in builds.items()}
        fns.update({"torch.fft": vendor, "copy": copy})
        ts = round_robin(fns, args.reps, alternate=True)      # every fn returns its own milliseconds
        q = {k: (v[len(v) // 4], v[len(v) // 2], v[(3 * len(v)) // 4]) for k, v in ts.items()}
        for k, v in ts.items():
            lo, med, hi = q[k]
            print(f"{k:20s} median {med:8.3f} ms  quartiles {lo:8.3f} {hi:8.3f}  min {v[0]:8.3f}  {moved / (med * 1e-3) / 1e12:6.3f} TB/s (in + out)  "
                  f"{med / q['copy'][1]:6.3f} x the copy", flush=True)
        b, t, c = q["bluestein"], q["torch.fft"], q["copy"]
        print(f"RATIO n={n}: bluestein / torch.fft = {b[1] / t[1]:.4f} (quartiles {b[0] / t[2]:.4f} ... {b[2] / t[0]:.4f}), "
              f"bluestein / copy = {b[1] / c[1]:.4f} (quartiles {b[0] / c[2]:.4f} ... {b[2] / c[0]:.4f})", flush=True)
        for name in builds:
            if name != "shipped":
                a = q[f"bluestein ({name})"]
                print(f"BUILDS n={n}: shipped {b[1]:.4f} ms, {name} {a[1]:.4f} ms, shipped / {name} = {b[1] / a[1]:.4f} (quartiles {b[0] / a[2]:.4f} ... {b[2] / a[0]:.4f})", flush=True)
        del plan


if __name__ == "__main__":
    main()

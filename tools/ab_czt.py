"""The chirp-z transforms (smfft_czt_benchmark) against what a caller had before them, on ONE buffer in ONE process, timed round robin so
that drift of the box hits all alike:
  czt:         smfft_czt_benchmark, one fused launch (the library's own events) -- the shipped build and every build given with --alt
               (plain instead of non-temporal row loads and stores: make -C smfft_amd/csrc EXTRA_HIPFLAGS=-DSMFFT_NT=0 CZT_LIB=...
               CZT_OBJDIR=... <that CZT_LIB>)
  bluestein:   smfft_bluestein_benchmark on the same buffers, where the job is the same one: m = n, start = 0, step = 1 / n.  The ratio
               is the price of the general kernel (two chirp tables, sixteen elements of a thread instead of eight)
  matmul:      torch.matmul(x, W, out=y) of the rows with the dense n x m complex64 matrix exp(-2 pi i j (start + k step)), between
               events: the only thing a torch user has for a zoom
  copy:        a copy_ of (in + out) / 2 bytes, between events: as many bytes read and written as the transform moves
Shapes: 4 GiB of complex64 in (2^29 elements; batch = 2^29 // n rows).  DFT: m = n = 1000, 2039.  ZOOM: (n, m) = (2048, 256), (1000, 24),
(1024, 1024) at start = 0.1, step = 1 / (8 n).  Every entry is warmed up twice; medians, quartiles and minima over --reps rounds, which
run through the entries forwards and backwards in turn.  Before the timing the fused output is compared with the other entry's and a
sample of rows with the fp64 sum of tools/czt_model.py.  RATIO lines: czt / bluestein, czt / matmul, czt / copy; BUILDS lines:
shipped / other build.
    python tools/ab_czt.py [--reps 20] [--alt NAME=lib.so ...] [--small] > profiles/r19_czt_ab.txt"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import smfft_amd as sm  # noqa: E402
from smfft_amd import bluestein, czt  # noqa: E402
import czt_model as cm  # noqa: E402  (beside this file)
from ab_fir_common import round_robin  # noqa: E402
from ab_fir_common import timed as events  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--alt", action="append", default=[], metavar="NAME=PATH", help="another build of libsmfft_czt.so")
    ap.add_argument("--small", action="store_true", help="a sixty-fourth of the buffer (a rehearsal, not a measurement)")
    args = ap.parse_args()
    sm.FFT_init()
    torch.cuda.init()
    stream = torch.cuda.current_stream()          # the default stream: smfft_czt_benchmark times on the null stream
    builds = {"shipped": czt.lib()}
    for item in args.alt:
        name, path = item.split("=", 1)
        builds[name] = czt.load(os.path.abspath(path))
    elements = (1 << 29) // (64 if args.small else 1)
    print(f"device: {torch.cuda.get_device_name(0)}; {args.reps} reps round robin; {elements * 8 / 2**30:.3f} GiB in; "
          f"builds of libsmfft_czt.so: {', '.join(builds)}", flush=True)
    gen = torch.Generator(device="cuda").manual_seed(0)
    x_all = torch.view_as_complex(torch.empty((elements, 2), dtype=torch.float32, device="cuda").normal_(generator=gen))
    y_all = torch.empty(elements, dtype=torch.complex64, device="cuda")
    y_ref = torch.empty(elements, dtype=torch.complex64, device="cuda")
    shapes = [("DFT", n, n, 0.0, 1.0 / n) for n in (1000, 2039)] + [("ZOOM", n, m, 0.1, 1.0 / (8 * n)) for n, m in ((2048, 256), (1000, 24), (1024, 1024))]
    for kind, n, m, start, step in shapes:
        batch = elements // n
        M = czt.fft_size(n, m)
        x = x_all[:batch * n].view(batch, n)
        y, yr = (t[:batch * m].view(batch, m) for t in (y_all, y_ref))
        plan = torch.empty(3 * M, dtype=torch.complex64, device="cuda")
        czt.prepare(n, m, start, step, plan.data_ptr())
        moved = batch * (n + m) * 8
        half = torch.empty(moved // 16, dtype=torch.complex64, device="cuda"), torch.empty(moved // 16, dtype=torch.complex64, device="cuda")
        print(f"--- {kind} n={n} m={m} M={M} start={start} step={step:.6g} batch={batch}: {-(-batch // (4096 // M))} tiles, "
              f"{moved / 2**30:.2f} GiB moved (in + out)", flush=True)

        def fused(lib):
            def run():
                t = ctypes.c_double(0.0)
                rc = lib.smfft_czt_benchmark(x.data_ptr(), y.data_ptr(), n, m, batch, plan.data_ptr(), ctypes.byref(t))
                assert rc == 0, rc
                return t.value
            return run

        def copy():
            return events(lambda: half[1].copy_(half[0]), stream)

        if kind == "DFT":
            bplan = torch.empty(2 * bluestein.fft_size(n), dtype=torch.complex64, device="cuda")
            bluestein.prepare(n, bplan.data_ptr())

            def other():
                t = ctypes.c_double(0.0)
                rc = bluestein.lib().smfft_bluestein_benchmark(x.data_ptr(), yr.data_ptr(), n, batch, bplan.data_ptr(), ctypes.byref(t))
                assert rc == 0, rc
                return t.value
            other_name = "bluestein"
        else:
            W = torch.from_numpy(cm.unit(-cm.phases(n, m, start, step)).astype(np.complex64)).cuda()

            def other():
                return events(lambda: torch.matmul(x, W, out=yr), stream)
            other_name = "matmul"

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
        other()
        torch.cuda.synchronize()
        scale = yr.abs().max().item()
        print(f"max |czt - {other_name}| / max |{other_name}| = {(y - yr).abs().max().item() / scale:.2e}", flush=True)
        rows = [0, batch // 2, batch - 1]
        want = cm.direct(x[rows].cpu().numpy(), m, start, step)
        for name, out in (("czt", y), (other_name, yr)):
            d = out[rows].cpu().numpy().astype(np.complex128) - want
            print(f"{name} vs the fp64 sum (rows {rows}): worst relL2 {np.max(np.linalg.norm(d, axis=1) / np.linalg.norm(want, axis=1)):.2e}", flush=True)

        fns = {("czt" if name == "shipped" else f"czt ({name})"): fused(lib) for name, lib in builds.items()}
        fns.update({other_name: other, "copy": copy})
        ts = round_robin(fns, args.reps, alternate=True)      # every fn returns its own milliseconds
        q = {k: (v[len(v) // 4], v[len(v) // 2], v[(3 * len(v)) // 4]) for k, v in ts.items()}
        for k, v in ts.items():
            lo, med, hi = q[k]
            print(f"{k:20s} median {med:8.3f} ms  quartiles {lo:8.3f} {hi:8.3f}  min {v[0]:8.3f}  {moved / (med * 1e-3) / 1e12:6.3f} TB/s (in + out)  "
                  f"{med / q['copy'][1]:6.3f} x the copy", flush=True)
        c, o, p = q["czt"], q[other_name], q["copy"]
        print(f"RATIO {kind} n={n} m={m}: czt / {other_name} = {c[1] / o[1]:.4f} (quartiles {c[0] / o[2]:.4f} ... {c[2] / o[0]:.4f}), "
              f"czt / copy = {c[1] / p[1]:.4f} (quartiles {c[0] / p[2]:.4f} ... {c[2] / p[0]:.4f})", flush=True)
        for name in builds:
            if name != "shipped":
                a = q[f"czt ({name})"]
                print(f"BUILDS {kind} n={n} m={m}: shipped {c[1]:.4f} ms, {name} {a[1]:.4f} ms, shipped / {name} = {c[1] / a[1]:.4f} "
                      f"(quartiles {c[0] / a[2]:.4f} ... {c[2] / a[0]:.4f})", flush=True)
        del plan, half


if __name__ == "__main__":
    main()

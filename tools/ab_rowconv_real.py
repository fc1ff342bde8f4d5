"""The real row-pair convolutions (smfft_rowconv_real_benchmark) against what a caller had before them, on ONE pair of buffers in ONE
process, timed round robin so that drift of the box hits all alike:
  real:            smfft_rowconv_real_benchmark, one fused launch (the library's own events) -- the shipped build and every build given
                   with --alt NAME=PATH: the partner on ds_bpermute instead of through LDS at M <= 1024 (make -C smfft_amd/csrc
                   ROWCONV_REAL_SPLIT=1 ROWCONV_REAL_LIB=... ROWCONV_REAL_OBJDIR=... <that ROWCONV_REAL_LIB>), plain instead of
                   non-temporal row loads and stores (EXTRA_HIPFLAGS=-DSMFFT_NT=0), and -- a name that starts with "timing" -- the
                   kernel without its balancing step (EXTRA_HIPFLAGS=-DSMFFT_TIMING_ONLY_ROWCONV_REAL_NO_BALANCE=1), which gives other
                   results, is compared with nothing and is never shipped: it prices the reductions
  complex:         smfft_rowconv_benchmark on the complex64 cast of the same rows, made beforehand
  cast + complex:  the two casts (torch copy_ of float32 into complex64) and smfft_rowconv_launch between events: what a caller with
                   real rows paid
  torch:           the unfused pipeline on real rows between events: torch.fft.rfft(a, n=M), torch.fft.rfft(b', n=M) (b' = b, or
                   b.flip(-1) in correlate mode), the product, torch.fft.irfft(n=M), the slice [first, first + m) copied out
  copy:            a copy_ of (a + b + out) / 2 bytes of the real launch, between events: as many bytes read and written as it moves
Shapes: 2 GiB of float32 of a (2^29 elements; batch = 2^29 // n_a rows, the row counts of profiles/r20_rowconv_ab.txt) and as many rows
of b, (n_a, n_b) = (1024, 1024), (2048, 2049), (4000, 97), (1000, 25); the full output and the window of the lags -16 ... 16
(first = n_b - 17, m = 33); both modes.  Every entry is warmed up twice; medians, quartiles and minima over --reps rounds, which run
through the entries forwards and backwards in turn.  Before the timing the real output is compared with the real part of the complex
kernel's and with the pipeline's and a sample of rows with the fp64 sum of tools/rowconv_real_model.py, and the builds with the
shipped one to the bit.  RATIO lines: real / complex, real / (cast + complex), real / torch, real / copy; BUILDS lines: shipped / other.
    python tools/ab_rowconv_real.py [--reps 20] [--alt NAME=lib.so ...] [--small] > profiles/r21_rowconv_real_ab.txt"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import smfft_amd as sm  # noqa: E402
from smfft_amd import rowconv, rowconv_real  # noqa: E402
import rowconv_real_model as rrm  # noqa: E402  (beside this file)
from ab_fir_common import round_robin  # noqa: E402
from ab_fir_common import timed as events  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--alt", action="append", default=[], metavar="NAME=PATH", help="another build of libsmfft_rowconv_real.so")
    ap.add_argument("--small", action="store_true", help="a sixty-fourth of the buffers (a rehearsal, not a measurement)")
    args = ap.parse_args()
    sm.FFT_init()
    torch.cuda.init()
    stream = torch.cuda.current_stream()          # the default stream: the benchmark entry points time on the null stream
    builds = {"shipped": rowconv_real.lib()}
    for item in args.alt:
        name, path = item.split("=", 1)
        builds[name] = rowconv_real.load(os.path.abspath(path))
    clib = rowconv.lib()
    elements = (1 << 29) // (64 if args.small else 1)
    print(f"device: {torch.cuda.get_device_name(0)}; {args.reps} reps round robin; {elements * 4 / 2**30:.3f} GiB of a; "
          f"builds of libsmfft_rowconv_real.so: {', '.join(builds)}", flush=True)
    gen = torch.Generator(device="cuda").manual_seed(0)
    a_all = torch.empty(elements, dtype=torch.float32, device="cuda").normal_(generator=gen)
    b_all = torch.empty(elements + elements // 1024, dtype=torch.float32, device="cuda").normal_(generator=gen)
    for n_a, n_b in ((1024, 1024), (2048, 2049), (4000, 97), (1000, 25)):
        batch = elements // n_a
        M = rowconv_real.fft_size(n_a, n_b)
        full = n_a + n_b - 1
        a, b = a_all[:batch * n_a].view(batch, n_a), b_all[:batch * n_b].view(batch, n_b)
        ac, bc = torch.empty((batch, n_a), dtype=torch.complex64, device="cuda"), torch.empty((batch, n_b), dtype=torch.complex64, device="cuda")
        ac.copy_(a), bc.copy_(b)
        y_all = torch.empty(batch * full, dtype=torch.float32, device="cuda")
        y_ref = torch.empty(batch * full, dtype=torch.float32, device="cuda")
        yc_all = torch.empty(batch * full, dtype=torch.complex64, device="cuda")
        for first, m in ((0, full), (n_b - 17, 33)):
            y, yr, yc = (t[:batch * m].view(batch, m) for t in (y_all, y_ref, yc_all))
            moved = batch * (n_a + n_b + m) * 4
            half = torch.empty(moved // 8, dtype=torch.float32, device="cuda"), torch.empty(moved // 8, dtype=torch.float32, device="cuda")
            for correlate in (0, 1):
                mode = "correlate" if correlate else "convolve"
                print(f"--- {mode} n_a={n_a} n_b={n_b} first={first} m={m} M={M} batch={batch}: {-(-batch // (4096 // M))} tiles, "
                      f"{moved / 2**30:.2f} GiB moved (a + b + out, float32)", flush=True)

                def fused(lib):
                    def run():
                        t = ctypes.c_double(0.0)
                        rc = lib.smfft_rowconv_real_benchmark(a.data_ptr(), b.data_ptr(), y.data_ptr(), n_a, n_b, first, m, batch, correlate, ctypes.byref(t))
                        assert rc == 0, rc
                        return t.value
                    return run

                def on_cast_rows():
                    t = ctypes.c_double(0.0)
                    rc = clib.smfft_rowconv_benchmark(ac.data_ptr(), bc.data_ptr(), yc.data_ptr(), n_a, n_b, first, m, batch, correlate, ctypes.byref(t))
                    assert rc == 0, rc
                    return t.value

                def cast_and_launch():
                    ac.copy_(a)
                    bc.copy_(b)
                    rc = clib.smfft_rowconv_launch(ac.data_ptr(), bc.data_ptr(), yc.data_ptr(), n_a, n_b, first, m, batch, correlate, None)
                    assert rc == 0, rc

                def pipeline():
                    second = b.flip(-1) if correlate else b
                    spectrum = torch.fft.rfft(a, n=M, dim=-1)
                    spectrum *= torch.fft.rfft(second, n=M, dim=-1)
                    yr.copy_(torch.fft.irfft(spectrum, n=M, dim=-1)[:, first:first + m])

                # the same results first
                base = None
                for name, lib in builds.items():
                    y.fill_(float("nan"))
                    fused(lib)()
                    if base is None:
                        base = y.clone()
                    elif not name.startswith("timing"):
                        assert torch.equal(y.view(torch.int32), base.view(torch.int32)), f"{name}: bits differ from the shipped build"
                y.copy_(base)
                del base
                on_cast_rows()
                events(pipeline, stream)
                torch.cuda.synchronize()
                scale = yr.abs().max().item()
                print(f"max |real - Re complex| / max = {(y - yc.real).abs().max().item() / scale:.2e}; max |real - torch| / max = {(y - yr).abs().max().item() / scale:.2e}", flush=True)
                rows = [0, batch // 2, batch - 1]
                want = rrm.direct(a[rows].cpu().numpy(), b[rows].cpu().numpy(), bool(correlate))
                norm = np.linalg.norm(want, axis=1) * np.sqrt(m / full)       # a window is judged against its share of the full row
                for name, out in (("real", y), ("complex", yc.real), ("torch", yr)):
                    d = out[rows].cpu().numpy().astype(np.float64) - want[:, first:first + m]
                    print(f"{name} vs the fp64 sum (rows {rows}): worst ||d|| / (||full want|| sqrt(m / Lfull)) {np.max(np.linalg.norm(d, axis=1) / norm):.2e}", flush=True)

                fns = {("real" if name == "shipped" else f"real ({name})"): fused(lib) for name, lib in builds.items()}
                fns.update({"complex": on_cast_rows, "cast + complex": lambda: events(cast_and_launch, stream), "torch": lambda: events(pipeline, stream),
                            "copy": lambda: events(lambda: half[1].copy_(half[0]), stream)})
                ts = round_robin(fns, args.reps, alternate=True)      # every fn returns its own milliseconds
                q = {k: (v[len(v) // 4], v[len(v) // 2], v[(3 * len(v)) // 4]) for k, v in ts.items()}
                for k, v in ts.items():
                    lo, med, hi = q[k]
                    print(f"{k:24s} median {med:8.3f} ms  quartiles {lo:8.3f} {hi:8.3f}  min {v[0]:8.3f}  {moved / (med * 1e-3) / 1e12:6.3f} TB/s (the real launch's bytes)  "
                          f"{med / q['copy'][1]:6.3f} x the copy", flush=True)
                c = q["real"]
                what = f"{mode} n_a={n_a} n_b={n_b} m={m}"
                print(f"RATIO {what}: " + ", ".join(f"real / {k} = {c[1] / o[1]:.4f} (quartiles {c[0] / o[2]:.4f} ... {c[2] / o[0]:.4f})"
                                                    for k, o in ((k, q[k]) for k in ("complex", "cast + complex", "torch", "copy"))), flush=True)
                for name in builds:
                    if name != "shipped":
                        alt = q[f"real ({name})"]
                        print(f"BUILDS {what}: shipped {c[1]:.4f} ms, {name} {alt[1]:.4f} ms, shipped / {name} = {c[1] / alt[1]:.4f} "
                              f"(quartiles {c[0] / alt[2]:.4f} ... {c[2] / alt[0]:.4f})", flush=True)
            del half
        del y_all, y_ref, yc_all, ac, bc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

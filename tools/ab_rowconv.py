"""The row-pair convolutions (smfft_rowconv_benchmark) against what a caller had before them, on ONE pair of buffers in ONE process, timed
round robin so that drift of the box hits all alike:
  rowconv:     smfft_rowconv_benchmark, one fused launch (the library's own events) -- the shipped build and every build given with
               --alt (plain instead of non-temporal row loads and stores: make -C smfft_amd/csrc EXTRA_HIPFLAGS=-DSMFFT_NT=0
               ROWCONV_LIB=... ROWCONV_OBJDIR=... <that ROWCONV_LIB>; b loaded behind the first transform instead of up front:
               EXTRA_HIPFLAGS=-DSMFFT_ROWCONV_LATE_B=1)
  torch:       the unfused pipeline between events: torch.fft.fft(a, n=M), torch.fft.fft(b', n=M) (both pad to M; b' = b, or
               b.flip(-1).conj() in correlate mode), the product, torch.fft.ifft, the slice [first, first + m) copied into the output
  copy:        a copy_ of (a + b + out) / 2 bytes, between events: as many bytes read and written as the fused launch moves
Shapes: 4 GiB of complex64 of a (2^29 elements; batch = 2^29 // n_a rows) and as many rows of b, (n_a, n_b) = (1024, 1024),
(2048, 2049), (4000, 97), (1000, 25); the full output and the window of the lags -16 ... 16 (first = n_b - 17, m = 33); both modes.
Every entry is warmed up twice; medians, quartiles and minima over --reps rounds, which run through the entries forwards and backwards
in turn.  Before the timing the fused output is compared with the pipeline's and a sample of rows with the fp64 sum of
tools/rowconv_model.py, and the builds with each other to the bit.  RATIO lines: rowconv / torch, rowconv / copy; BUILDS lines:
shipped / other build.
    python tools/ab_rowconv.py [--reps 20] [--alt NAME=lib.so ...] [--small] > profiles/r20_rowconv_ab.txt"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import smfft_amd as sm  # noqa: E402
from smfft_amd import rowconv  # noqa: E402
import rowconv_model as rm  # noqa: E402  (beside this file)
from ab_fir_common import round_robin  # noqa: E402
from ab_fir_common import timed as events  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--alt", action="append", default=[], metavar="NAME=PATH", help="another build of libsmfft_rowconv.so")
    ap.add_argument("--small", action="store_true", help="a sixty-fourth of the buffers (a rehearsal, not a measurement)")
    args = ap.parse_args()
    sm.FFT_init()
    torch.cuda.init()
    stream = torch.cuda.current_stream()          # the default stream: smfft_rowconv_benchmark times on the null stream
    builds = {"shipped": rowconv.lib()}
    for item in args.alt:
        name, path = item.split("=", 1)
        builds[name] = rowconv.load(os.path.abspath(path))
    elements = (1 << 29) // (64 if args.small else 1)
    print(f"device: {torch.cuda.get_device_name(0)}; {args.reps} reps round robin; {elements * 8 / 2**30:.3f} GiB of a; "
          f"builds of libsmfft_rowconv.so: {', '.join(builds)}", flush=True)
    gen = torch.Generator(device="cuda").manual_seed(0)
    a_all = torch.view_as_complex(torch.empty((elements, 2), dtype=torch.float32, device="cuda").normal_(generator=gen))
    b_all = torch.view_as_complex(torch.empty((elements + elements // 1024, 2), dtype=torch.float32, device="cuda").normal_(generator=gen))
    for n_a, n_b in ((1024, 1024), (2048, 2049), (4000, 97), (1000, 25)):
        batch = elements // n_a
        M = rowconv.fft_size(n_a, n_b)
        full = n_a + n_b - 1
        a, b = a_all[:batch * n_a].view(batch, n_a), b_all[:batch * n_b].view(batch, n_b)
        y_all = torch.empty(batch * full, dtype=torch.complex64, device="cuda")
        y_ref = torch.empty(batch * full, dtype=torch.complex64, device="cuda")
        for first, m in ((0, full), (n_b - 17, 33)):
            y, yr = (t[:batch * m].view(batch, m) for t in (y_all, y_ref))
            moved = batch * (n_a + n_b + m) * 8
            half = torch.empty(moved // 16, dtype=torch.complex64, device="cuda"), torch.empty(moved // 16, dtype=torch.complex64, device="cuda")
            for correlate in (0, 1):
                mode = "correlate" if correlate else "convolve"
                print(f"--- {mode} n_a={n_a} n_b={n_b} first={first} m={m} M={M} batch={batch}: {-(-batch // (4096 // M))} tiles, "
                      f"{moved / 2**30:.2f} GiB moved (a + b + out)", flush=True)

                def fused(lib):
                    def run():
                        t = ctypes.c_double(0.0)
                        rc = lib.smfft_rowconv_benchmark(a.data_ptr(), b.data_ptr(), y.data_ptr(), n_a, n_b, first, m, batch, correlate, ctypes.byref(t))
                        assert rc == 0, rc
                        return t.value
                    return run

                def pipeline():
                    second = b.flip(-1).conj() if correlate else b
                    spectrum = torch.fft.fft(a, n=M, dim=-1)
                    spectrum *= torch.fft.fft(second, n=M, dim=-1)
                    yr.copy_(torch.fft.ifft(spectrum, dim=-1)[:, first:first + m])

                def other():
                    return events(pipeline, stream)

                def copy():
                    return events(lambda: half[1].copy_(half[0]), stream)

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
                print(f"max |rowconv - torch| / max |torch| = {(y - yr).abs().max().item() / scale:.2e}", flush=True)
                rows = [0, batch // 2, batch - 1]
                want = rm.direct(a[rows].cpu().numpy(), b[rows].cpu().numpy(), bool(correlate))
                norm = np.linalg.norm(want, axis=1) * np.sqrt(m / full)       # a window is judged against its share of the full row
                for name, out in (("rowconv", y), ("torch", yr)):
                    d = out[rows].cpu().numpy().astype(np.complex128) - want[:, first:first + m]
                    print(f"{name} vs the fp64 sum (rows {rows}): worst ||d|| / (||full want|| sqrt(m / Lfull)) {np.max(np.linalg.norm(d, axis=1) / norm):.2e}", flush=True)

                fns = {("rowconv" if name == "shipped" else f"rowconv ({name})"): fused(lib) for name, lib in builds.items()}
                fns.update({"torch": other, "copy": copy})
                ts = round_robin(fns, args.reps, alternate=True)      # every fn returns its own milliseconds
                q = {k: (v[len(v) // 4], v[len(v) // 2], v[(3 * len(v)) // 4]) for k, v in ts.items()}
                for k, v in ts.items():
                    lo, med, hi = q[k]
                    print(f"{k:20s} median {med:8.3f} ms  quartiles {lo:8.3f} {hi:8.3f}  min {v[0]:8.3f}  {moved / (med * 1e-3) / 1e12:6.3f} TB/s (a + b + out)  "
                          f"{med / q['copy'][1]:6.3f} x the copy", flush=True)
                c, o, p = q["rowconv"], q["torch"], q["copy"]
                what = f"{mode} n_a={n_a} n_b={n_b} m={m}"
                print(f"RATIO {what}: rowconv / torch = {c[1] / o[1]:.4f} (quartiles {c[0] / o[2]:.4f} ... {c[2] / o[0]:.4f}), "
                      f"rowconv / copy = {c[1] / p[1]:.4f} (quartiles {c[0] / p[2]:.4f} ... {c[2] / p[0]:.4f})", flush=True)
                for name in builds:
                    if name != "shipped":
                        alt = q[f"rowconv ({name})"]
                        print(f"BUILDS {what}: shipped {c[1]:.4f} ms, {name} {alt[1]:.4f} ms, shipped / {name} = {c[1] / alt[1]:.4f} "
                              f"(quartiles {c[0] / alt[2]:.4f} ... {c[2] / alt[0]:.4f})", flush=True)
            del half
        del y_all, y_ref
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

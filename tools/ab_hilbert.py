"""The Hilbert kernels (smfft_hilbert_benchmark) against their other builds and against what a caller had before them, on ONE pair of
buffers in ONE process, timed round robin so that drift of the box hits all alike:
  hilbert: smfft_hilbert_benchmark, one fused launch (the library's own events) -- the shipped build and every build given with
           --alt NAME=PATH: x kept in registers across the transforms instead of loaded a second time in front of the store, or the
           other way round (make -C smfft_amd/csrc HILBERT_KEEP_X=1 HILBERT_LIB=... HILBERT_OBJDIR=... <that HILBERT_LIB>), plain
           instead of non-temporal row loads and stores (EXTRA_HIPFLAGS="-DSMFFT_HILBERT_NT_LOAD=0 -DSMFFT_HILBERT_NT_STORE=0", or one
           of the two).  All builds must give the same bits
  torch:   the unfused pipeline on the same buffers between events: torch.fft.fft of the rows (complex, full length), the mask
           -i s[k], torch.fft.ifft, and .imag (kind 0), its sum with x as a complex tensor (kind 1) or the modulus of that (kind 2)
  copy:    a copy_ of the kind's own bytes (n floats in and n floats -- kind 1: n complex64 -- out per row), between events
Shapes: 2 GiB of float32 input (2^29 elements) as rows of n = 512 ... 8192 (--lengths: others), the three kinds.  Every entry is
warmed up twice; medians, quartiles and minima over --reps rounds, which run through the entries forwards and backwards in turn (the
method of DESIGN.md section 21).  Before the timing the output is compared with the pipeline's and a sample of rows with the fp64
chain of tools/hilbert_model.py, and the builds with the shipped one to the bit.  RATIO lines: hilbert / torch, hilbert / copy;
BUILDS lines: shipped / other.
    python tools/ab_hilbert.py [--reps 15] [--lengths 512 1024 2048 4096 8192] [--kinds 0 1 2] [--alt NAME=lib.so ...] [--small] > profiles/r23_hilbert_ab.txt"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import smfft_amd as sm  # noqa: E402
from smfft_amd import hilbert  # noqa: E402
import hilbert_model as hm  # noqa: E402  (beside this file)
from ab_fir_common import round_robin  # noqa: E402
from ab_fir_common import timed as events  # noqa: E402

NAMES = {0: "quadrature", 1: "analytic", 2: "envelope"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--alt", action="append", default=[], metavar="NAME=PATH", help="another build of libsmfft_hilbert.so")
    ap.add_argument("--lengths", type=int, nargs="+", default=[512, 1024, 2048, 4096, 8192], help="the row lengths n")
    ap.add_argument("--kinds", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--no-torch", action="store_true", help="leave the unfused pipeline out (builds against each other and the copy)")
    ap.add_argument("--small", action="store_true", help="a sixty-fourth of the buffers (a rehearsal, not a measurement)")
    args = ap.parse_args()
    sm.FFT_init()
    torch.cuda.init()
    stream = torch.cuda.current_stream()          # the default stream: the benchmark entry point times on the null stream
    builds = {"shipped": hilbert.lib()}
    for item in args.alt:
        name, path = item.split("=", 1)
        builds[name] = hilbert.load(os.path.abspath(path))
    elements = (1 << 29) // (64 if args.small else 1)
    print(f"device: {torch.cuda.get_device_name(0)}; {args.reps} reps round robin; {elements * 4 / 2**30:.3f} GiB of input; "
          f"builds of libsmfft_hilbert.so: {', '.join(builds)}", flush=True)
    gen = torch.Generator(device="cuda").manual_seed(0)
    x_all = torch.empty(elements, dtype=torch.float32, device="cuda").normal_(generator=gen)
    y_all = torch.empty(2 * elements, dtype=torch.float32, device="cuda")         # the analytic kind writes two floats per sample
    y_ref = torch.empty(2 * elements, dtype=torch.float32, device="cuda")
    spare = torch.empty(2 * elements, dtype=torch.float32, device="cuda")
    same_bits = True
    for n in args.lengths:
        batch = elements // n
        M = n // 2
        x = x_all.view(batch, n)
        mask = torch.zeros(n, dtype=torch.complex64, device="cuda")
        mask[1:M] = -1j
        mask[M + 1:] = 1j
        for kind in args.kinds:
            width = 2 if kind == 1 else 1
            y, yr = y_all[:width * elements], y_ref[:width * elements]
            moved = (1 + width) * batch * n * 4
            what = f"{NAMES[kind]} n={n}"
            print(f"--- {what} M={M} batch={batch}: {-(-batch // (4096 // M))} tiles, {moved / 2**30:.2f} GiB moved (in + out)", flush=True)

            def fused(lib):
                def run():
                    t = ctypes.c_double(0.0)
                    rc = lib.smfft_hilbert_benchmark(x.data_ptr(), y.data_ptr(), n, batch, kind, ctypes.byref(t))
                    assert rc == 0, rc
                    return t.value
                return run

            def pipeline():
                # in slabs of 2^26 samples, so that the complex workspaces of the full length fit beside the buffers
                rows = max(1, (1 << 26) // n)
                for first in range(0, batch, rows):
                    xs = x[first:first + rows]
                    spectrum = torch.fft.fft(xs, dim=-1)
                    spectrum *= mask
                    h = torch.fft.ifft(spectrum, dim=-1).real
                    if kind == 0:
                        yr.view(batch, n)[first:first + rows].copy_(h)
                    elif kind == 1:
                        torch.view_as_complex(yr.view(batch, n, 2))[first:first + rows].copy_(torch.complex(xs, h))
                    else:
                        torch.abs(torch.complex(xs, h), out=yr.view(batch, n)[first:first + rows])

            # the same results first
            base = None
            for name, lib in builds.items():
                y.fill_(float("nan"))
                fused(lib)()
                if base is None:
                    base = y.clone()
                else:
                    differ = int((y.view(torch.int32) != base.view(torch.int32)).sum().item())
                    print(f"{name}: {differ} of {y.numel()} outputs differ from the shipped build's bits", flush=True)
                    same_bits = same_bits and differ == 0
            del base
            shape = lambda t: torch.view_as_complex(t.view(batch, n, 2)) if kind == 1 else t.view(batch, n)  # noqa: E731
            rows = [0, batch // 2, batch - 1]
            xs = x[rows].cpu().numpy()
            want = hm.chain(xs, kind)
            outs = [("hilbert", y)]
            if not args.no_torch:
                events(pipeline, stream)
                torch.cuda.synchronize()
                print(f"max |hilbert - torch| / max = {(y - yr).abs().max().item() / yr.abs().max().item():.2e}", flush=True)
                outs.append(("torch", yr))
            for name, out in outs:
                l2, mx = hm.errors(shape(out)[rows].cpu().numpy(), want, xs)
                print(f"{name} vs the fp64 chain (rows {rows}): worst row relL2 {l2:.2e}, max |d| / max |x| {mx:.2e}", flush=True)

            fns = {("hilbert" if name == "shipped" else f"hilbert ({name})"): fused(lib) for name, lib in builds.items()}
            if not args.no_torch:
                fns["torch"] = lambda: events(pipeline, stream)
            ncopy = (1 + width) * elements // 2       # a copy that moves the launch's bytes: it reads ncopy floats and writes as many
            fns["copy"] = lambda: events(lambda: spare[:ncopy].copy_(y_ref[:ncopy]), stream)
            ts = round_robin(fns, args.reps, alternate=True)      # every fn returns its own milliseconds
            q = {k: (v[len(v) // 4], v[len(v) // 2], v[(3 * len(v)) // 4]) for k, v in ts.items()}
            for k, v in ts.items():
                lo, med, hi = q[k]
                print(f"{k:24s} median {med:8.3f} ms  quartiles {lo:8.3f} {hi:8.3f}  min {v[0]:8.3f}  {moved / (med * 1e-3) / 1e12:6.3f} TB/s (the launch's bytes)  "
                      f"{med / q['copy'][1]:6.3f} x the copy", flush=True)
            c = q["hilbert"]
            print(f"RATIO {what}: " + ", ".join(f"hilbert / {k} = {c[1] / o[1]:.4f} (quartiles {c[0] / o[2]:.4f} ... {c[2] / o[0]:.4f})"
                                                for k, o in ((k, q[k]) for k in ("torch", "copy") if k in q)), flush=True)
            for name in builds:
                if name != "shipped":
                    alt = q[f"hilbert ({name})"]
                    sep = "separate" if c[2] < alt[0] or alt[2] < c[0] else "overlap: tie"
                    print(f"BUILDS {what}: shipped {c[1]:.4f} ms (quartiles {c[0]:.4f} ... {c[2]:.4f}), {name} {alt[1]:.4f} ms (quartiles {alt[0]:.4f} ... {alt[2]:.4f}), "
                          f"shipped / {name} = {c[1] / alt[1]:.4f}; quartile ranges {sep}", flush=True)
        torch.cuda.empty_cache()
    assert same_bits, "a build's bits differ from the shipped build's (see above)"


if __name__ == "__main__":
    main()

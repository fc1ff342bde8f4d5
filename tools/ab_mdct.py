"""The DCT-IV / MDCT / IMDCT kernels (smfft_dct4_benchmark, smfft_mdct_benchmark, smfft_imdct_benchmark) against their other builds and
against what a caller had before them, on ONE set of buffers in ONE process, timed round robin so that drift of the box hits all alike:
  fused:   the library's benchmark entry point, one fused launch (the library's own events) -- the shipped build and every build given
           with --alt NAME=PATH: the row accesses as 4-byte accesses at stride two instead of 16-byte accesses and a pass through LDS
           (make -C smfft_amd/csrc MDCT_STAGED=0 MDCT_LIB=... MDCT_OBJDIR=... <that MDCT_LIB>), and the row accesses plain instead of
           non-temporal or the other way round (MDCT_NT=0 / MDCT_NT=1).  All builds must give the same bits
  torch:   the unfused pipeline on the same buffers between events: the index permutation t = x[2p] + i x[n-1-2p], the twiddle
           product, torch.fft.fft, the second twiddle product, the real and the imaginary part copied out interleaved; for the MDCT
           the window product and the fold in front of that, for the IMDCT the unfold and the window product behind it
  copy:    a copy_ of the launch's bytes (input + output floats), between events
Shapes: 2 GiB of float32 input (2^29 elements) as rows of n = 512, 2048 and 8192 (--lengths: others): rows of n for dct4, frames of 2 N
for the MDCT (a sine window), rows of N for the IMDCT.  Every entry is warmed up twice; medians, quartiles and minima over --reps
rounds, which run through the entries forwards and backwards in turn (the method of DESIGN.md section 21).  Before the timing the
output is compared with the pipeline's and a sample of rows with the fp64 chain of tools/mdct_model.py, and the builds with the
shipped one to the bit.  RATIO lines: fused / torch, fused / copy; BUILDS lines: shipped / other.
    python tools/ab_mdct.py [--reps 15] [--lengths 512 1024 2048 4096 8192] [--alt NAME=lib.so ...] [--small] > profiles/r24_mdct_ab.txt"""
import argparse
import ctypes
import math
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import smfft_amd as sm  # noqa: E402
from smfft_amd import mdct  # noqa: E402
import mdct_model as mm  # noqa: E402  (beside this file)
from ab_fir_common import round_robin  # noqa: E402
from ab_fir_common import timed as events  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--alt", action="append", default=[], metavar="NAME=PATH", help="another build of libsmfft_mdct.so")
    ap.add_argument("--lengths", type=int, nargs="+", default=[512, 2048, 8192], help="the row lengths n (N)")
    ap.add_argument("--kinds", nargs="+", default=["dct4", "mdct", "imdct"])
    ap.add_argument("--small", action="store_true", help="a sixty-fourth of the buffers (a rehearsal, not a measurement)")
    args = ap.parse_args()
    sm.FFT_init()
    torch.cuda.init()
    stream = torch.cuda.current_stream()          # the default stream: the benchmark entry points time on the null stream
    builds = {"shipped": mdct.lib()}
    for item in args.alt:
        name, path = item.split("=", 1)
        builds[name] = mdct.load(os.path.abspath(path))
    elements = (1 << 29) // (64 if args.small else 1)
    print(f"device: {torch.cuda.get_device_name(0)}; {args.reps} reps round robin; {elements * 4 / 2**30:.3f} GiB of input; "
          f"builds of libsmfft_mdct.so: {', '.join(builds)}", flush=True)
    gen = torch.Generator(device="cuda").manual_seed(0)
    x_all = torch.empty(elements, dtype=torch.float32, device="cuda").normal_(generator=gen)
    y_all = torch.empty(2 * elements, dtype=torch.float32, device="cuda")
    y_ref = torch.empty(2 * elements, dtype=torch.float32, device="cuda")
    spare = torch.empty(3 * elements, dtype=torch.float32, device="cuda")
    same_bits = True
    for n in args.lengths:
        M = n // 2
        p = torch.arange(M, device="cuda", dtype=torch.float64)
        pre = torch.polar(torch.ones_like(p), -math.pi * (4 * p + 1) / (4 * n)).to(torch.complex64)
        post = torch.polar(torch.ones_like(p), -math.pi * p / n).to(torch.complex64)
        w = mdct.sine_window(n, "cuda")
        i0, s0, i1, s1 = (torch.from_numpy(a).cuda() for a in mm.fold_index(n))
        s0, s1 = s0.float(), s1.float()
        ui, us = (torch.from_numpy(a).cuda() for a in mm.unfold_index(n))
        us = us.float() * w

        def core(u, scale, out):
            """out[:, 2k] = scale Re Y[k], out[:, n-1-2k] = -scale Im Y[k] of the rows u of n floats"""
            spectrum = torch.fft.fft(torch.complex(u[:, 0::2], u.flip(-1)[:, 0::2]) * pre, dim=-1)
            spectrum *= post
            torch.mul(spectrum.real, scale, out=out[:, 0::2])
            torch.mul(spectrum.imag.flip(-1), -scale, out=out[:, 1::2])

        for kind in args.kinds:
            nin, nout = (2 * n if kind == "mdct" else n), (2 * n if kind == "imdct" else n)
            batch = elements // nin
            x, y, yr = x_all.view(batch, nin), y_all[:batch * nout].view(batch, nout), y_ref[:batch * nout].view(batch, nout)
            moved = batch * (nin + nout) * 4
            print(f"--- {kind} n={n} M={M} batch={batch}: {-(-batch // (4096 // M))} tiles, {moved / 2**30:.2f} GiB moved (in + out, float32)", flush=True)

            def fused(lib):
                def run():
                    t = ctypes.c_double(0.0)
                    if kind == "dct4":
                        rc = lib.smfft_dct4_benchmark(x.data_ptr(), y.data_ptr(), n, batch, 0, ctypes.byref(t))
                    elif kind == "mdct":
                        rc = lib.smfft_mdct_benchmark(x.data_ptr(), y.data_ptr(), w.data_ptr(), n, batch, 1, n, 2 * n, ctypes.byref(t))
                    else:
                        rc = lib.smfft_imdct_benchmark(x.data_ptr(), y.data_ptr(), w.data_ptr(), n, batch, ctypes.byref(t))
                    assert rc == 0, rc
                    return t.value
                return run

            def pipeline():
                if kind == "dct4":
                    core(x, 2.0, yr)
                elif kind == "mdct":
                    v = x * w
                    core(s0 * v[:, i0] + s1 * v[:, i1], 1.0, yr)
                else:
                    D = torch.empty_like(x)
                    core(x, 1.0, D)
                    torch.mul(D[:, ui], us, out=yr)

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
            print(f"max |fused - torch| / max = {(y - yr).abs().max().item() / yr.abs().max().item():.2e}", flush=True)
            rows = [0, batch // 2, batch - 1]
            xs, wh = x[rows].cpu().numpy(), w.cpu().numpy()
            want = mm.chain(xs) if kind == "dct4" else mm.mdct_chain(xs, wh) if kind == "mdct" else mm.imdct_chain(xs, wh)
            for name, out in (("fused", y), ("torch", yr)):
                l2, mx = mm.errors(out[rows].cpu().numpy(), want)
                print(f"{name} vs the fp64 chain (rows {rows}): worst row relL2 {l2:.2e}, max |d| / max |want| {mx:.2e}", flush=True)

            words = batch * (nin + nout) // 2
            fns = {("fused" if name == "shipped" else f"fused ({name})"): fused(lib) for name, lib in builds.items()}
            fns.update({"torch": lambda: events(pipeline, stream), "copy": lambda: events(lambda: spare[:words].copy_(spare[words:2 * words]), stream)})
            ts = round_robin(fns, args.reps, alternate=True)      # every fn returns its own milliseconds
            q = {k: (v[len(v) // 4], v[len(v) // 2], v[(3 * len(v)) // 4]) for k, v in ts.items()}
            for k, v in ts.items():
                lo, med, hi = q[k]
                print(f"{k:24s} median {med:8.3f} ms  quartiles {lo:8.3f} {hi:8.3f}  min {v[0]:8.3f}  {moved / (med * 1e-3) / 1e12:6.3f} TB/s (the launch's bytes)  "
                      f"{med / q['copy'][1]:6.3f} x the copy", flush=True)
            c = q["fused"]
            what = f"{kind} n={n}"
            print(f"RATIO {what}: " + ", ".join(f"fused / {k} = {c[1] / o[1]:.4f} (quartiles {c[0] / o[2]:.4f} ... {c[2] / o[0]:.4f})"
                                                for k, o in ((k, q[k]) for k in ("torch", "copy"))), flush=True)
            for name in builds:
                if name != "shipped":
                    alt = q[f"fused ({name})"]
                    sep = "separate" if c[2] < alt[0] or alt[2] < c[0] else "overlap: tie"
                    print(f"BUILDS {what}: shipped {c[1]:.4f} ms (quartiles {c[0]:.4f} ... {c[2]:.4f}), {name} {alt[1]:.4f} ms (quartiles {alt[0]:.4f} ... {alt[2]:.4f}), "
                          f"shipped / {name} = {c[1] / alt[1]:.4f}; quartile ranges {sep}", flush=True)
            torch.cuda.empty_cache()
    assert same_bits, "a build's bits differ from the shipped build's (see above)"


if __name__ == "__main__":
    main()

"""The STFT kernels (smfft_stft_benchmark, smfft_istft_benchmark) against their other build and against what a caller had before them,
on ONE set of buffers in ONE process, timed round robin so that drift of the box hits all alike:
  fused:   the library's benchmark entry point, one fused launch (the library's own events) -- the shipped build and every build given
           with --alt NAME=PATH: the sample loads and the stores plain instead of non-temporal or the other way round
           (make -C smfft_amd/csrc STFT_NT=0 STFT_LIB=... STFT_OBJDIR=... <that STFT_LIB>).  All builds must give the same bits
  torch:   the unfused pipeline on the same buffers between events: torch.stft(center=False, onesided=True) -- the gather of the
           frames, the window product and the rfft -- and, for the power, abs() ** 2 behind it; for the inverse torch.fft.irfft
           and the window product
  copy:    a copy_ of the bytes the kernel itself moves (the signal once + the output; the spectra + the frames for the inverse),
           between events
Shapes: 2 GiB of float32 signal (2^29 samples) as 64 streams, in frames of n = 512 ... 8192 at hop = n / 4 and hop = n under the periodic
Hann window, both kinds; the inverse on the rows of bins that 2 GiB of output frames take.  Every entry is warmed up twice; medians,
quartiles and minima over --reps rounds, which run through the entries forwards and backwards in turn (the method of DESIGN.md
section 21).  Before the timing the output is compared with the pipeline's and a sample of frames with the fp64 chain of
tools/stft_model.py, and the builds with the shipped one to the bit.  RATIO lines: fused / torch, fused / copy; BUILDS lines:
shipped / other.
    python tools/ab_stft.py [--reps 15] [--lengths 512 1024 2048 4096 8192] [--alt NAME=lib.so ...] [--small] > profiles/r25_stft_ab.txt"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import smfft_amd as sm  # noqa: E402
from smfft_amd import stft  # noqa: E402
import stft_model as mm  # noqa: E402  (beside this file)
from ab_fir_common import round_robin  # noqa: E402
from ab_fir_common import timed as events  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--alt", action="append", default=[], metavar="NAME=PATH", help="another build of libsmfft_stft.so")
    ap.add_argument("--lengths", type=int, nargs="+", default=[512, 1024, 2048, 4096, 8192], help="the frame lengths n")
    ap.add_argument("--kinds", nargs="+", default=["complex", "power", "inverse"])
    ap.add_argument("--small", action="store_true", help="a sixty-fourth of the buffers (a rehearsal, not a measurement)")
    args = ap.parse_args()
    sm.FFT_init()
    torch.cuda.init()
    stream = torch.cuda.current_stream()          # the default stream: the benchmark entry points time on the null stream
    builds = {"shipped": stft.lib()}
    for item in args.alt:
        name, path = item.split("=", 1)
        builds[name] = stft.load(os.path.abspath(path))
    elements = (1 << 29) // (64 if args.small else 1)
    C = 64
    L = elements // C
    print(f"device: {torch.cuda.get_device_name(0)}; {args.reps} reps round robin; {elements * 4 / 2**30:.3f} GiB of signal as {C} streams of {L} samples; "
          f"builds of libsmfft_stft.so: {', '.join(builds)}", flush=True)
    gen = torch.Generator(device="cuda").manual_seed(0)
    signal = torch.empty((C, L), dtype=torch.float32, device="cuda").normal_(generator=gen)
    same_bits = True
    for n in args.lengths:
        M = n // 2
        w = stft.hann(n, "cuda")
        cases = [(kind, hop) for kind in args.kinds if kind != "inverse" for hop in (n // 4, n)] + [("inverse", None)] * ("inverse" in args.kinds)
        for kind, hop in cases:
            if kind == "inverse":
                batch = elements // n
                x = torch.view_as_complex(torch.empty((batch, M + 1, 2), dtype=torch.float32, device="cuda").normal_(generator=gen))
                y, yr = torch.empty((batch, n), dtype=torch.float32, device="cuda"), torch.empty((batch, n), dtype=torch.float32, device="cuda")
                moved = batch * ((M + 1) * 8 + n * 4)
                what = f"inverse n={n}"
                print(f"--- {what} M={M} batch={batch}: {-(-batch // (4096 // M))} tiles, {moved / 2**30:.2f} GiB moved (bins in + frames out)", flush=True)
            else:
                F = 1 + (L - n) // hop
                dtype = torch.complex64 if kind == "complex" else torch.float32
                y, yr = torch.empty((C, F, M + 1), dtype=dtype, device="cuda"), None
                moved = elements * 4 + y.numel() * y.element_size()
                what = f"{kind} n={n} hop={hop}"
                print(f"--- {what} M={M}: {C} streams of {F} frames, {-(-C * F // (4096 // M))} tiles, {moved / 2**30:.2f} GiB moved (the signal once + the output); "
                      f"the framed copy torch makes is {C * F * n * 4 / 2**30:.2f} GiB", flush=True)

            def fused(lib):
                def run():
                    t = ctypes.c_double(0.0)
                    if kind == "inverse":
                        rc = lib.smfft_istft_benchmark(x.data_ptr(), y.data_ptr(), w.data_ptr(), n, batch, ctypes.byref(t))
                    else:
                        rc = lib.smfft_stft_benchmark(signal.data_ptr(), y.data_ptr(), w.data_ptr(), n, C, F, hop, L, int(kind == "power"), ctypes.byref(t))
                    assert rc == 0, rc
                    return t.value
                return run

            def pipeline():
                if kind == "inverse":
                    torch.mul(torch.fft.irfft(x, n, dim=-1), w, out=yr)
                    return yr
                X = torch.stft(signal, n, hop, window=w, center=False, onesided=True, return_complex=True)
                return X if kind == "complex" else X.abs() ** 2

            # the same results first
            base = None
            for name, lib in builds.items():
                (torch.view_as_real(y) if y.is_complex() else y).fill_(float("nan"))
                fused(lib)()
                if base is None:
                    base = y.clone()
                else:
                    a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (y, base))
                    differ = int((a.view(torch.int32) != b.view(torch.int32)).sum().item())
                    print(f"{name}: {differ} of {a.numel()} output floats differ from the shipped build's bits", flush=True)
                    same_bits = same_bits and differ == 0
            del base
            ref = pipeline()
            torch.cuda.synchronize()
            if kind != "inverse":
                ref = ref.transpose(-1, -2)                  # torch.stft returns (streams, M + 1, frames)
            print(f"max |fused - torch| / max = {(y - ref).abs().max().item() / ref.abs().max().item():.2e}", flush=True)
            if kind == "inverse":
                rows = [0, batch // 2, batch - 1]
                want = mm.inverse_chain(x[rows].cpu().numpy(), w.cpu().numpy())
                outs = (("fused", y[rows]), ("torch", ref[rows]))
            else:
                picks = [(0, 0), (C // 2, F // 2), (C - 1, F - 1)]
                xs = torch.stack([signal[c, f * hop:f * hop + n] for c, f in picks]).cpu().numpy()
                want = mm.chain(xs, w.cpu().numpy(), power=kind == "power")
                outs = (("fused", torch.stack([y[c, f] for c, f in picks])), ("torch", torch.stack([ref[c, f] for c, f in picks])))
            for name, out in outs:
                l2, mx = mm.errors(out.cpu().numpy(), want)
                print(f"{name} vs the fp64 chain (3 frames): worst row relL2 {l2:.2e}, max |d| / max |want| {mx:.2e}", flush=True)
            del ref
            torch.cuda.empty_cache()

            words = moved // 8
            spare = torch.empty(2 * words, dtype=torch.float32, device="cuda")
            fns = {("fused" if name == "shipped" else f"fused ({name})"): fused(lib) for name, lib in builds.items()}
            fns.update({"torch": lambda: events(pipeline, stream), "copy": lambda: events(lambda: spare[:words].copy_(spare[words:]), stream)})
            ts = round_robin(fns, args.reps, alternate=True)      # every fn returns its own milliseconds
            q = {k: (v[len(v) // 4], v[len(v) // 2], v[(3 * len(v)) // 4]) for k, v in ts.items()}
            for k, v in ts.items():
                lo, med, hi = q[k]
                print(f"{k:24s} median {med:8.3f} ms  quartiles {lo:8.3f} {hi:8.3f}  min {v[0]:8.3f}  {moved / (med * 1e-3) / 1e12:6.3f} TB/s (the launch's bytes)  "
                      f"{med / q['copy'][1]:6.3f} x the copy", flush=True)
            c = q["fused"]
            print(f"RATIO {what}: " + ", ".join(f"fused / {k} = {c[1] / o[1]:.4f} (quartiles {c[0] / o[2]:.4f} ... {c[2] / o[0]:.4f})"
                                                for k, o in ((k, q[k]) for k in ("torch", "copy"))), flush=True)
            for name in builds:
                if name != "shipped":
                    alt = q[f"fused ({name})"]
                    sep = "separate" if c[2] < alt[0] or alt[2] < c[0] else "overlap: tie"
                    print(f"BUILDS {what}: shipped {c[1]:.4f} ms (quartiles {c[0]:.4f} ... {c[2]:.4f}), {name} {alt[1]:.4f} ms (quartiles {alt[0]:.4f} ... {alt[2]:.4f}), "
                          f"shipped / {name} = {c[1] / alt[1]:.4f}; quartile ranges {sep}", flush=True)
            del spare, y, yr
            if kind == "inverse":
                del x
            torch.cuda.empty_cache()
    assert same_bits, "a build's bits differ from the shipped build's (see above)"


if __name__ == "__main__":
    main()

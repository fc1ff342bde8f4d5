"""The Welch kernels (smfft_welch_benchmark, smfft_csd_benchmark) against their other builds and against what a caller had before them,
on ONE set of buffers in ONE process, timed round robin so that drift of the box hits all alike:
  fused:   the library's benchmark entry points, one fused launch each (the library's own events) -- the shipped build and every build
           given with --alt NAME=PATH: non-temporal sample loads, the window kept in registers, the next frame's loads in front of the
           transform (make -C smfft_amd/csrc WELCH_NT=1 | WELCH_KEEP_WINDOW=1 | WELCH_PREFETCH=1 WELCH_LIB=... WELCH_OBJDIR=...
           <that WELCH_LIB>).  All builds must give the same bits
  stft+sum:   the unfused pipeline for the auto spectra on the same buffers between events: smfft_stft_launch(kind = 1) into a buffer of
              all frames' powers and torch.sum over the frames of each group
  2stft+mul+sum: the unfused pipeline for the cross spectra: two smfft_stft_launch(kind = 0), conj(X) * Y and torch.sum
  copy:    a copy_ of the signal's bytes (one signal; the cross spectra read two), between events: the floor
Shapes: 2 GiB of float32 signal (2^29 samples) as 64 streams (and as much again for y), in frames of n = 512 ... 8192 at hop = n / 4 and
hop = n under the periodic Hann window, T = 8, 64 and smfft_amd.welch.default_T.  Every entry is warmed up twice; medians, quartiles and
minima over --reps rounds, which run through the entries forwards and backwards in turn (the method of DESIGN.md section 21).  Before
the timing the fused outputs are compared with the pipelines' and the builds with the shipped one to the bit.  RATIO lines:
fused / pipeline and fused / copy, with "separate" where the quartile ranges do not overlap and "overlap: tie" where they do; BUILDS
lines: shipped / other; T lines: the T of the sweep that took the least time per shape.
    python tools/ab_welch.py [--reps 15] [--lengths 512 ... 8192] [--alt NAME=lib.so ...] [--small] > profiles/r27_welch_ab.txt"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import smfft_amd as sm  # noqa: E402
from smfft_amd import stft, welch  # noqa: E402
from ab_fir_common import round_robin  # noqa: E402  (beside this file)
from ab_fir_common import timed as events  # noqa: E402


def quartiles(v):
    return v[len(v) // 4], v[len(v) // 2], v[(3 * len(v)) // 4]


def verdict(a, b):
    return "separate" if a[2] < b[0] or b[2] < a[0] else "overlap: tie"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--alt", action="append", default=[], metavar="NAME=PATH", help="another build of libsmfft_welch.so")
    ap.add_argument("--lengths", type=int, nargs="+", default=[512, 1024, 2048, 4096, 8192], help="the frame lengths n")
    ap.add_argument("--small", action="store_true", help="a sixty-fourth of the buffers (a rehearsal, not a measurement)")
    args = ap.parse_args()
    sm.FFT_init()
    torch.cuda.init()
    stream = torch.cuda.current_stream()          # the default stream: the benchmark entry points time on the null stream
    builds = {"shipped": welch.lib()}
    for item in args.alt:
        name, path = item.split("=", 1)
        builds[name] = welch.load(os.path.abspath(path))
    elements = (1 << 29) // (64 if args.small else 1)
    C = 64
    L = elements // C
    print(f"device: {torch.cuda.get_device_name(0)}; {args.reps} reps round robin; {elements * 4 / 2**30:.3f} GiB of signal as {C} streams of {L} samples "
          f"(and as much for y); builds of libsmfft_welch.so: {', '.join(builds)}", flush=True)
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.empty((C, L), dtype=torch.float32, device="cuda").normal_(generator=gen)
    y = torch.empty((C, L), dtype=torch.float32, device="cuda").normal_(generator=gen).mul_(0.5)
    y[:, 3:].add_(x[:, :-3], alpha=0.7)
    spare = torch.empty((C, L), dtype=torch.float32, device="cuda")
    same_bits = True
    wins = {}                                     # (kernel, M) -> {build: shapes at which its median was the least}
    for n in args.lengths:
        M = n // 2
        w = stft.hann(n, "cuda")
        for hop in (n // 4, n):
            F = 1 + (L - n) // hop
            P = torch.empty((C, F, M + 1), dtype=torch.float32, device="cuda")
            X, Y = (torch.empty((C, F, M + 1), dtype=torch.complex64, device="cuda") for _ in range(2))
            XY = torch.empty_like(X)
            best_T = {}
            sweep = []
            for T in (8, 64, welch.default_T(C, F, n)):
                if T not in sweep and F // T:
                    sweep.append(T)
            for T in sweep:
                G = F // T
                what = f"n={n} hop={hop} T={T}" + (" (default_T)" if T == welch.default_T(C, F, n) else "")
                print(f"--- {what} M={M}: {C} streams of {G} groups ({F} frames), {-(-C * G // (4096 // M))} tiles; the frames' powers are "
                      f"{P.numel() * 4 / 2**30:.2f} GiB, their spectra {X.numel() * 8 / 2**30:.2f} GiB per signal; the output {C * G * (M + 1) * 4 / 2**20:.2f} MiB", flush=True)
                S = torch.empty((C, G, M + 1), dtype=torch.float32, device="cuda")
                Sc = torch.empty((C, G, M + 1), dtype=torch.complex64, device="cuda")

                def fused(lib, cross):
                    def run():
                        t = ctypes.c_double(0.0)
                        if cross:
                            rc = lib.smfft_csd_benchmark(x.data_ptr(), y.data_ptr(), Sc.data_ptr(), w.data_ptr(), n, C, G, T, hop, L, L, ctypes.byref(t))
                        else:
                            rc = lib.smfft_welch_benchmark(x.data_ptr(), S.data_ptr(), w.data_ptr(), n, C, G, T, hop, L, ctypes.byref(t))
                        assert rc == 0, rc
                        return t.value
                    return run

                def auto_pipeline():
                    stft.launch_ptr(x.data_ptr(), P.data_ptr(), w.data_ptr(), n, C, F, hop, L, power=True)
                    return P[:, :G * T].view(C, G, T, M + 1).sum(dim=2)

                def cross_pipeline():
                    stft.launch_ptr(x.data_ptr(), X.data_ptr(), w.data_ptr(), n, C, F, hop, L)
                    stft.launch_ptr(y.data_ptr(), Y.data_ptr(), w.data_ptr(), n, C, F, hop, L)
                    torch.mul(torch.conj_physical(X), Y, out=XY)
                    return XY[:, :G * T].view(C, G, T, M + 1).sum(dim=2)

                # the same results first
                for cross, out in ((False, S), (True, Sc)):
                    base = None
                    for name, lib in builds.items():
                        (torch.view_as_real(out) if cross else out).fill_(float("nan"))
                        fused(lib, cross)()
                        if base is None:
                            base = out.clone()
                        else:
                            a, b = (torch.view_as_real(t) if cross else t for t in (out, base))
                            differ = int((a.view(torch.int32) != b.view(torch.int32)).sum().item())
                            print(f"{'csd' if cross else 'welch'} ({name}): {differ} of {a.numel()} output floats differ from the shipped build's bits", flush=True)
                            same_bits = same_bits and differ == 0
                    ref = cross_pipeline() if cross else auto_pipeline()
                    torch.cuda.synchronize()
                    print(f"{'csd' if cross else 'welch'}: max |fused - pipeline| / max = {(base - ref).abs().max().item() / ref.abs().max().item():.2e}", flush=True)
                    del ref, base
                fns = {}
                for name, lib in builds.items():
                    fns[f"welch ({name})"] = fused(lib, False)
                    fns[f"csd ({name})"] = fused(lib, True)
                fns["stft+sum"] = lambda: events(auto_pipeline, stream)
                fns["2stft+mul+sum"] = lambda: events(cross_pipeline, stream)
                fns["copy"] = lambda: events(lambda: spare.copy_(x), stream)
                ts = round_robin(fns, args.reps, alternate=True)      # every fn returns its own milliseconds
                q = {k: quartiles(v) for k, v in ts.items()}
                for k, v in ts.items():
                    lo, med, hi = q[k]
                    print(f"{k:24s} median {med:8.3f} ms  quartiles {lo:8.3f} {hi:8.3f}  min {v[0]:8.3f}  {med / q['copy'][1]:6.3f} x the copy of one signal", flush=True)
                for kernel, pipeline in (("welch", "stft+sum"), ("csd", "2stft+mul+sum")):
                    c, o, cp = q[f"{kernel} (shipped)"], q[pipeline], q["copy"]
                    print(f"RATIO {kernel} {what}: fused / {pipeline} = {c[1] / o[1]:.4f} (quartiles {c[0] / o[2]:.4f} ... {c[2] / o[0]:.4f}; {verdict(c, o)}), "
                          f"fused / copy = {c[1] / cp[1]:.4f}", flush=True)
                    for name in builds:
                        if name != "shipped":
                            alt = q[f"{kernel} ({name})"]
                            print(f"BUILDS {kernel} {what}: shipped {c[1]:.4f} ms (quartiles {c[0]:.4f} ... {c[2]:.4f}), {name} {alt[1]:.4f} ms (quartiles {alt[0]:.4f} ... "
                                  f"{alt[2]:.4f}), shipped / {name} = {c[1] / alt[1]:.4f}; quartile ranges {verdict(c, alt)}", flush=True)
                    least = min(builds, key=lambda name: q[f"{kernel} ({name})"][1])
                    wins.setdefault((kernel, M), {}).setdefault(least, []).append(f"hop={hop} T={T}")
                    best_T.setdefault(kernel, []).append((c[1] * F / (G * T), T))     # per frame that was summed
                del S, Sc
            for kernel, times in best_T.items():
                print(f"T {kernel} n={n} hop={hop}: " + ", ".join(f"T={T}: {ms:.3f} ms" for ms, T in times) + f" (scaled to all {F} frames); least at T={min(times)[1]}; "
                      f"default_T = {welch.default_T(C, F, n)}", flush=True)
            del P, X, Y, XY
            torch.cuda.empty_cache()
    for (kernel, M), tally in sorted(wins.items()):
        print(f"WINS {kernel} M={M}: " + "; ".join(f"{name}: {len(shapes)} of {sum(len(s) for s in tally.values())} shapes" for name, shapes in tally.items()), flush=True)
    assert same_bits, "a build's bits differ from the shipped build's (see above)"


if __name__ == "__main__":
    main()

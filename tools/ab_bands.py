"""The band-spectrogram kernel (smfft_bands_benchmark) against its other builds and against what a caller had before it, on ONE set of
buffers in ONE process, timed round robin so that drift of the box hits all alike:
  fused:        the library's benchmark entry point, one fused launch (the library's own events) -- the shipped build and every build
                given with --alt NAME=PATH: the plan read from global memory per frame, non-temporal sample loads (make -C
                smfft_amd/csrc BANDS_STAGE_PLAN=0 | BANDS_NT=1 BANDS_LIB=... BANDS_OBJDIR=... <that BANDS_LIB>).  All builds must give
                the same bits: neither switch touches the arithmetic or its order
  stft+matmul:  (a) the unfused pipeline on the same buffers between events: smfft_stft_launch(kind = 1) into a workspace of all
                frames' powers and torch.matmul with the dense (M + 1) x bands filter bank
  torch:        (b) torch.stft -> abs() ** 2 -> matmul with the same bank
  copy:         (c) a copy_ of as many bytes as the kernel moves (the signal read once, the output written once), between events
  welch:        (d) smfft_welch_benchmark on the same frames in groups of T = 64: the frames' transforms with next to no store
Shapes: 2 GiB of float32 signal (2^29 samples) as 64 streams, in frames of n = 512 ... 8192 at hop = n / 4 and hop = n under the
periodic Hann window, HTK mel tables at 16 kHz with 80 and 128 bands.  Every entry is warmed up twice; medians, quartiles and minima
over --reps rounds, which run through the entries forwards and backwards in turn (the method of DESIGN.md section 21).  Before the
timing the fused output is compared with the pipeline's and the builds with the shipped one to the bit.  RATIO lines: fused / each of
(a) ... (d), with "separate" where the quartile ranges do not overlap and "overlap: tie" where they do; BUILDS lines: shipped / other.
    python tools/ab_bands.py [--reps 15] [--lengths 512 ... 8192] [--mels 80 128] [--alt NAME=lib.so ...] [--small] > profiles/r28_bands_ab.txt"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import smfft_amd as sm  # noqa: E402
from smfft_amd import bands, stft, welch  # noqa: E402
from ab_fir_common import round_robin  # noqa: E402  (beside this file)
from ab_fir_common import timed as events  # noqa: E402


def quartiles(v):
    return v[len(v) // 4], v[len(v) // 2], v[(3 * len(v)) // 4]


def verdict(a, b):
    return "separate" if a[2] < b[0] or b[2] < a[0] else "overlap: tie"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--alt", action="append", default=[], metavar="NAME=PATH", help="another build of libsmfft_bands.so")
    ap.add_argument("--lengths", type=int, nargs="+", default=[512, 1024, 2048, 4096, 8192], help="the frame lengths n")
    ap.add_argument("--mels", type=int, nargs="+", default=[80, 128], help="the band counts of the HTK mel tables")
    ap.add_argument("--small", action="store_true", help="a sixty-fourth of the buffers (a rehearsal, not a measurement)")
    ap.add_argument("--no-torch", action="store_true", help="leave out (b), torch.stft -> abs() ** 2 -> matmul")
    args = ap.parse_args()
    sm.FFT_init()
    torch.cuda.init()
    stream = torch.cuda.current_stream()          # the default stream: the benchmark entry points time on the null stream
    builds = {"shipped": bands.lib()}
    for item in args.alt:
        name, path = item.split("=", 1)
        builds[name] = bands.load(os.path.abspath(path))
    elements = (1 << 29) // (64 if args.small else 1)
    C = 64
    L = elements // C
    print(f"device: {torch.cuda.get_device_name(0)}; {args.reps} reps round robin; {elements * 4 / 2**30:.3f} GiB of signal as {C} streams of {L} samples; "
          f"builds of libsmfft_bands.so: {', '.join(builds)}", flush=True)
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.empty((C, L), dtype=torch.float32, device="cuda").normal_(generator=gen)
    spare = torch.empty((C, L), dtype=torch.float32, device="cuda")
    same_bits = True
    for n in args.lengths:
        M = n // 2
        w = stft.hann(n, "cuda")
        for hop in (n // 4, n):
            F = 1 + (L - n) // hop
            P = torch.empty((C, F, M + 1), dtype=torch.float32, device="cuda")
            T = min(64, F)                        # (fewer than 64 frames per stream: the rehearsal's buffers)
            S = torch.empty((C, F // T, M + 1), dtype=torch.float32, device="cuda")
            for n_mels in args.mels:
                dense = bands.mel_filterbank(n, 16000, n_mels)
                plan = bands.prepare(n, *bands.from_dense(n, dense))
                Wt = torch.from_numpy(dense.T.astype("float32")).cuda().contiguous()            # (M + 1, bands)
                out = torch.empty((C, F, n_mels), dtype=torch.float32, device="cuda")
                moved = (C * L + out.numel()) // 2
                what = f"n={n} hop={hop} mel={n_mels}"
                print(f"--- {what} M={M}: {C} streams of {F} frames, {-(-C * F // (4096 // M))} tiles; {plan.weights} weights, longest band {int(plan.count.max())}; "
                      f"the frames' powers are {P.numel() * 4 / 2**30:.2f} GiB, the output {out.numel() * 4 / 2**20:.2f} MiB", flush=True)

                def fused(lib):
                    def run():
                        t = ctypes.c_double(0.0)
                        rc = lib.smfft_bands_benchmark(x.data_ptr(), out.data_ptr(), w.data_ptr(), plan.tensor.data_ptr(), n, plan.bands, plan.weights, C, F, hop, L,
                                                       ctypes.byref(t))
                        assert rc == 0, rc
                        return t.value
                    return run

                def pipeline():
                    stft.launch_ptr(x.data_ptr(), P.data_ptr(), w.data_ptr(), n, C, F, hop, L, power=True)
                    return torch.matmul(P, Wt)

                def torch_pipeline():
                    X = torch.stft(x, n, hop_length=hop, window=w, center=False, return_complex=True)      # (C, M + 1, F)
                    return torch.matmul((X.abs() ** 2).transpose(1, 2), Wt)

                def welch_floor():
                    t = ctypes.c_double(0.0)
                    rc = welch.lib().smfft_welch_benchmark(x.data_ptr(), S.data_ptr(), w.data_ptr(), n, C, F // T, T, hop, L, ctypes.byref(t))
                    assert rc == 0, rc
                    return t.value

                # the same results first
                base = None
                for name, lib in builds.items():
                    out.fill_(float("nan"))
                    fused(lib)()
                    if base is None:
                        base = out.clone()
                    else:
                        differ = int((out.view(torch.int32) != base.view(torch.int32)).sum().item())
                        print(f"bands ({name}): {differ} of {out.numel()} output floats differ from the shipped build's bits", flush=True)
                        same_bits = same_bits and differ == 0
                ref = pipeline()
                torch.cuda.synchronize()
                print(f"bands: max |fused - stft+matmul| / max = {(base - ref).abs().max().item() / ref.abs().max().item():.2e}", flush=True)
                del ref, base
                fns = {f"bands ({name})": fused(lib) for name, lib in builds.items()}
                fns["stft+matmul"] = lambda: events(pipeline, stream)
                if not args.no_torch:
                    fns["torch"] = lambda: events(torch_pipeline, stream)
                fns["copy"] = lambda: events(lambda: spare.view(-1)[:moved].copy_(x.view(-1)[:moved]), stream)
                fns["welch"] = welch_floor
                ts = round_robin(fns, args.reps, alternate=True)      # every fn returns its own milliseconds
                q = {k: quartiles(v) for k, v in ts.items()}
                for k, v in ts.items():
                    lo, med, hi = q[k]
                    print(f"{k:24s} median {med:8.3f} ms  quartiles {lo:8.3f} {hi:8.3f}  min {v[0]:8.3f}", flush=True)
                c = q["bands (shipped)"]
                for other in ("stft+matmul", "torch", "copy", "welch"):
                    if other in q:
                        o = q[other]
                        print(f"RATIO {what}: fused / {other} = {c[1] / o[1]:.4f} (quartiles {c[0] / o[2]:.4f} ... {c[2] / o[0]:.4f}; {verdict(c, o)})", flush=True)
                for name in builds:
                    if name != "shipped":
                        alt = q[f"bands ({name})"]
                        print(f"BUILDS {what}: shipped {c[1]:.4f} ms (quartiles {c[0]:.4f} ... {c[2]:.4f}), {name} {alt[1]:.4f} ms (quartiles {alt[0]:.4f} ... "
                              f"{alt[2]:.4f}), shipped / {name} = {c[1] / alt[1]:.4f}; quartile ranges {verdict(c, alt)}", flush=True)
                del out, Wt, plan
            del P, S
            torch.cuda.empty_cache()
    assert same_bits, "a build's bits differ from the shipped build's (see above)"


if __name__ == "__main__":
    main()

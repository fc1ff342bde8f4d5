"""The overlap-save filter bank with N = 8192 / 16384 segments (smfft_large_fir_launch) against the same result built from public
pieces, in one process, timed round robin so that drift of the box hits all alike:
  fused:      smfft_large_fir_launch -- segment load, forward FFT, product, inverse FFT, the valid windows stored, one kernel
  unfused:    torch frames the segments into a contiguous (C S, N) buffer -> smfft_amd.large.launch forward -> torch broadcast
              multiply by the K spectra -> smfft_amd.large.launch inverse on K C S transforms -> torch gathers the windows into (C, K, L)
  torch-only: the same pipeline with torch.fft.fft / ifft
  old path:   smfft_fir_launch at N = 4096 with the same taps (when M <= 4095): what the filter banks could already do
  c2c:        smfft_amd.large.launch on as many transforms as the fused kernel does (2 C S K), for the per-transform comparison
  recompute:  (N = 8192, with --ab LIB) the form of the filter loop the library does not use there for K > 1 (one forward transform
              per (segment, filter) pair at two workgroups per CU; the shipped held form does one per segment at one), from an A/B
              build of the library:
              make -C smfft_amd/csrc LARGE_OBJDIR=../../build_ab/large_fir_recompute EXTRA_HIPFLAGS=-DSMFFT_LARGE_FIR_HELD_8192=0 \
                   LARGE_FIR_LIB=../../build_ab/libsmfft_large_fir_recompute.so ../../build_ab/libsmfft_large_fir_recompute.so
Main configurations: C = 1, L = 2^24, K = 32, (N, M) = (8192, 2049) and (16384, 4097), the output once from smfft_malloc_written_for
and once from plain hipMalloc (torch's allocator).  Sweep (fused only, plain output): K in {1, 8, 32, 128} at both lengths.  Per line:
median / min ms over the reps, the HBM floor (C L + C K L) * 8 B / 8 TB/s, and the fp32 rate at 5 N log2 N flop per transform as a
fraction of FP32_PEAK_TFLOPS (bench.py).
    python tools/ab_large_fir.py [--reps 30] [--ab LIB] [--no-sweep]
    python tools/ab_large_fir.py --trace DIR      (one fused launch per main configuration under rocprofv3 --kernel-trace --stats)"""
import argparse
import ctypes
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
from ab_fir_common import as_tensor, round_robin  # noqa: E402  (beside this file; imports torch on first use)

FP32_PEAK_TFLOPS = 157.3     # bench.py
HBM_TBS = 8.0
MAIN = ((8192, 2049), (16384, 4097))


def report(name, v, C, L, K, N, transforms):
    med = v[len(v) // 2]
    floor = (C * L + C * K * L) * 8 / (HBM_TBS * 1e12) * 1e3
    flop = transforms * 5 * N * math.log2(N)
    frac = flop / (med * 1e-3) / 1e12 / FP32_PEAK_TFLOPS
    print(f"{name:46s} median {med:8.3f} ms  min {v[0]:8.3f}  max {v[-1]:8.3f}  HBM floor {floor:6.3f} ms ({floor / med:.2f} of it)  "
          f"{transforms:7d} transforms = {frac:.3f} of fp32 peak, {med * 1e6 / transforms:6.1f} ns each (whole chip)", flush=True)
    return med


def main_config(torch, sm, large, lf, N, M, args, rng):
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    C, L, K = 1, 1 << 24, 32
    V = N - M + 1
    S = -(-L // V)
    x = torch.from_numpy((rng.standard_normal((C, L)) + 1j * rng.standard_normal((C, L))).astype(np.complex64)).cuda()
    h = torch.from_numpy((rng.standard_normal((K, M)) + 1j * rng.standard_normal((K, M))).astype(np.complex64) / 64).cuda()
    H = torch.empty((K, N), dtype=torch.complex64, device="cuda")
    lf.prepare(h.data_ptr(), H.data_ptr(), M, K, N, "convolve", stream=sp)
    frames = torch.empty((C * S, N), dtype=torch.complex64, device="cuda")
    spec = torch.empty_like(frames)
    prod = torch.empty((K, C * S, N), dtype=torch.complex64, device="cuda")
    ys = torch.empty_like(prod)
    plain = torch.empty((C, K, L), dtype=torch.complex64, device="cuda")
    out_bytes = C * K * L * 8
    pw = ctypes.c_void_p()
    assert sm.lib.smfft_malloc_written_for(ys.data_ptr(), out_bytes, ctypes.byref(pw)) == 0
    placed = as_tensor(pw.value, (C, K, L))
    xpad = torch.zeros((C, (S - 1) * V + N), dtype=torch.complex64, device="cuda")
    xpad[:, M - 1:M - 1 + L] = x

    def fused(out, lib=None):
        if lib is None:
            return lambda: lf.launch(x.data_ptr(), L, C, H.data_ptr(), K, M, N, out.data_ptr(), "convolve", stream=sp)
        return lambda: lib.smfft_large_fir_launch(x.data_ptr(), L, C, H.data_ptr(), K, M, N, 0, out.data_ptr(), sp)

    def gather(out):
        out.copy_(ys.view(K, C, S, N)[..., M - 1:].reshape(K, C, S * V)[..., :L].permute(1, 0, 2))

    def unfused(out):
        def run():
            frames.view(C, S, N).copy_(xpad.unfold(1, N, V))
            large.launch(frames.data_ptr(), spec.data_ptr(), N, C * S, False, stream=sp)
            torch.mul(spec.unsqueeze(0), H.unsqueeze(1), out=prod)            # (1/N is folded into H)
            large.launch(prod.data_ptr(), ys.data_ptr(), N, K * C * S, True, stream=sp)
            gather(out)
        return run

    def torch_only(out):
        def run():
            frames.view(C, S, N).copy_(xpad.unfold(1, N, V))
            torch.fft.fft(frames, out=spec)
            torch.mul(spec.unsqueeze(0), H.unsqueeze(1), out=prod)
            torch.fft.ifft(prod, norm="forward", out=ys)
            gather(out)
        return run

    fns = {"fused      (smfft_malloc_written_for output)": fused(placed), "fused      (hipMalloc output)": fused(plain),
           "unfused    (smfft_malloc_written_for output)": unfused(placed), "unfused    (hipMalloc output)": unfused(plain),
           "torch-only (hipMalloc output)": torch_only(plain)}
    # the fused kernel's transforms: one forward per (segment, filter group) in the held form (N = 8192, K > 1: one group per segment
    # once C S reaches the CU count), one per (segment, filter) in the recompute form
    fused_transforms = C * S * (1 + K) if N == 8192 else 2 * C * S * K
    transforms = {n: (fused_transforms if n.startswith("fused") else C * S * (1 + K)) for n in fns}
    ab = lf.load(args.ab) if args.ab and N == 8192 else None
    if ab is not None:
        fns["recompute  (A/B build, hipMalloc output)"] = fused(plain, ab)
        transforms["recompute  (A/B build, hipMalloc output)"] = 2 * C * S * K
    nc2c = 2 * C * S * K
    if nc2c * N * 8 <= prod.numel() * 8 * 2:
        fns["c2c        (2 C S K transforms)"] = lambda: (large.launch(prod.data_ptr(), ys.data_ptr(), N, C * S * K, False, stream=sp),
                                                        large.launch(ys.data_ptr(), prod.data_ptr(), N, C * S * K, True, stream=sp))
        transforms["c2c        (2 C S K transforms)"] = nc2c
    if M <= 4095:
        H4 = torch.empty((K, 4096), dtype=torch.complex64, device="cuda")
        sm.fir_prepare(h.data_ptr(), H4.data_ptr(), M, K, 4096, "convolve", stream=sp)
        S4 = -(-L // (4096 - M + 1))
        fns["old path   (smfft_fir_launch, N = 4096)"] = lambda: sm.fir_launch(x.data_ptr(), L, C, H4.data_ptr(), K, M, 4096, plain.data_ptr(), "convolve", stream=sp)
        transforms["old path   (smfft_fir_launch, N = 4096)"] = C * S4 * (1 + K)
    # all compute the same thing: compare fused with unfused, held and numpy on a sampled window
    fns["unfused    (smfft_malloc_written_for output)"]()
    fns["fused      (hipMalloc output)"]()
    torch.cuda.synchronize()
    d = (plain - placed).abs().max().item() / placed.abs().max().item()
    n0, W = L - 5000, 5000
    xs = x[0, n0 - (M - 1):].cpu().numpy().astype(np.complex128)
    want = np.convolve(xs, h[K - 1].cpu().numpy().astype(np.complex128))[M - 1:M - 1 + W]
    got = plain[0, K - 1, n0:].cpu().numpy()
    print(f"N={N}: max |fused - unfused| / max |unfused| = {d:.2e};  fused vs np.convolve (last row, last {W}): "
          f"relL2 {np.linalg.norm(got - want) / np.linalg.norm(want):.2e}", flush=True)
    if ab is not None:
        fused(placed, ab)()
        torch.cuda.synchronize()
        print(f"N={N}: recompute form (A/B build) bit-identical to the shipped held form: "
              f"{bool(torch.equal(torch.view_as_real(plain), torch.view_as_real(placed)))}", flush=True)
    print(f"main configuration: C={C} L=2^24 K={K} M={M} N={N} (V={V}, S={S}), output {out_bytes / 2**30:.0f} GiB, {args.reps} reps round robin", flush=True)
    ts = round_robin(fns, args.reps, stream)
    med = {}
    for name, v in ts.items():
        n = 4096 if name.startswith("old path") else N
        med[name] = report(name, v, C, L, K, n, transforms[name])
    for where in ("smfft_malloc_written_for output", "hipMalloc output"):
        print(f"  speed-up fused over unfused, {where}: {med[f'unfused    ({where})'] / med[f'fused      ({where})']:.2f} x", flush=True)
    print(f"  speed-up fused over torch-only: {med['torch-only (hipMalloc output)'] / med['fused      (hipMalloc output)']:.2f} x", flush=True)
    del frames, spec, prod, ys, xpad, placed, plain, fns
    sm.lib.smfft_free_written(pw.value)
    torch.cuda.empty_cache()
    return x


def sweep(torch, lf, x, N, M, args, rng):
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    C, L = x.shape
    S = -(-L // (N - M + 1))
    for K in (1, 8, 32, 128):
        h = torch.from_numpy((rng.standard_normal((K, M)) + 1j * rng.standard_normal((K, M))).astype(np.complex64)).cuda()
        H = torch.empty((K, N), dtype=torch.complex64, device="cuda")
        lf.prepare(h.data_ptr(), H.data_ptr(), M, K, N, "convolve", stream=sp)
        out = torch.empty((C, K, L), dtype=torch.complex64, device="cuda")
        fn = (lambda H=H, K=K, out=out: lf.launch(x.data_ptr(), L, C, H.data_ptr(), K, M, N, out.data_ptr(), "convolve", stream=sp))
        v = round_robin({"f": fn}, args.reps, stream)["f"]
        report(f"N={N:5d} M={M:4d} K={K:3d}", v, C, L, K, N, C * S * (1 + K) if N == 8192 and K > 1 else 2 * C * S * K)
        del out, H, h
        torch.cuda.empty_cache()


def once():
    """one prepare and one fused launch per main configuration: the program of the --trace run"""
    import smfft_amd as sm
    from smfft_amd import large_fir as lf
    sm.FFT_init()
    rng = np.random.default_rng(0)
    C, L, K = 1, 1 << 24, 32
    x = (rng.standard_normal((C, L)) + 1j * rng.standard_normal((C, L))).astype(np.complex64)
    dx = sm.DeviceBuffer.from_host(x)
    dout = sm.DeviceBuffer(C * K * L * 8)
    for N, M in MAIN:
        h = (rng.standard_normal((K, M)) + 1j * rng.standard_normal((K, M))).astype(np.complex64)
        dh, dspec = sm.DeviceBuffer.from_host(h), sm.DeviceBuffer(K * N * 8)
        lf.prepare(dh.ptr, dspec.ptr, M, K, N)
        for _ in range(3):
            lf.launch(dx.ptr, L, C, dspec.ptr, K, M, N, dout.ptr)
        assert sm.lib.smfft_synchronize() == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--ab", default=None, help="an A/B build of the library with the recompute form at N = 8192 for every K")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--only", type=int, default=0, help="one length only")
    ap.add_argument("--trace", default=None, help="output directory of a rocprofv3 --kernel-trace --stats run of --once")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    if args.once:
        return once()
    if args.trace:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", args.trace, "--", sys.executable, os.path.abspath(__file__), "--once"]
        return subprocess.check_call(cmd)
    import torch
    import smfft_amd as sm
    from smfft_amd import large, large_fir as lf
    sm.FFT_init()
    torch.cuda.init()
    rng = np.random.default_rng(0)
    for N, M in MAIN:
        if args.only and N != args.only:
            continue
        x = main_config(torch, sm, large, lf, N, M, args, rng)
        if not args.no_sweep:
            print(f"sweep (fused, hipMalloc output, C=1, L=2^24, N={N}, M={M}):", flush=True)
            sweep(torch, lf, x, N, M, args, rng)
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

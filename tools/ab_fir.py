"""The overlap-save filter bank (smfft_fir_launch) against the same result built from the library's public pieces, in one process, timed
round robin so that drift of the box hits all alike:
  fused:    smfft_fir_launch -- segment load, one forward FFT per segment, K products and inverse FFTs, the valid windows stored
  unfused:  torch frames the segments into a contiguous (C S, N) buffer -> smfft_launch forward external transform -> torch broadcast
            multiply by the K spectra -> smfft_launch inverse on K C S transforms -> torch gathers the valid windows into (C, K, L)
Main configuration: C = 1, L = 2^24, K = 32, M = 257, N = 1024 (V = 768, a 4 GiB output), the output once from smfft_malloc_written_for
and once from plain hipMalloc (torch's allocator).  Sweep (fused only, plain output): K in {1, 8, 32, 128}, N in {256, 1024, 4096},
M = N/4 + 1.  Per configuration: median / min ms over the reps, the HBM floor (C L + C K L) * 8 B / 8 TB/s, and the fp32 rate at
5 N log2 N flop per transform (forward transforms x filter groups + inverse transforms) as a fraction of FP32_PEAK_TFLOPS (bench.py).
    python tools/ab_fir.py [reps=9]"""
import ctypes
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import smfft_amd as sm  # noqa: E402
from ab_fir_common import as_tensor, round_robin  # noqa: E402  (beside this file)

FP32_PEAK_TFLOPS = 157.3     # bench.py
HBM_TBS = 8.0
TARGET_WORKGROUPS = 2048     # smfft_fir_kernel.hpp, kFirTargetWorkgroups
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 9


def groups_of(tiles, K):
    g = min(K, max(1, -(-TARGET_WORKGROUPS // tiles)))
    return -(-K // -(-K // g))


def transforms(C, L, K, N, M):
    S = -(-L // (N - M + 1))
    tiles = -(-(C * S) // (4096 // N))
    return C * S * (groups_of(tiles, K) + K)


def report(name, v, C, L, K, N, M):
    med = v[len(v) // 2]
    floor = (C * L + C * K * L) * 8 / (HBM_TBS * 1e12) * 1e3
    flop = transforms(C, L, K, N, M) * 5 * N * math.log2(N)
    frac = flop / (med * 1e-3) / 1e12 / FP32_PEAK_TFLOPS
    print(f"{name:44s} median {med:8.3f} ms  min {v[0]:8.3f}  HBM floor {floor:6.3f} ms ({floor / med:.2f} of it)  "
          f"{flop / 1e9:7.1f} GFLOP = {frac:.3f} of fp32 peak", flush=True)
    return med


def main():
    sm.FFT_init()
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    rng = np.random.default_rng(0)

    # ---------------------------------------------------------------- main configuration: fused vs unfused, two output placements
    C, L, K, M, N = 1, 1 << 24, 32, 257, 1024
    V = N - M + 1
    S = -(-L // V)
    x = torch.from_numpy((rng.standard_normal((C, L)) + 1j * rng.standard_normal((C, L))).astype(np.complex64)).cuda()
    h = torch.from_numpy((rng.standard_normal((K, M)) + 1j * rng.standard_normal((K, M))).astype(np.complex64) / 16).cuda()
    H = torch.empty((K, N), dtype=torch.complex64, device="cuda")
    sm.fir_prepare(h.data_ptr(), H.data_ptr(), M, K, N, "convolve", stream=sp)
    frames = torch.empty((C * S, N), dtype=torch.complex64, device="cuda")
    spec = torch.empty_like(frames)
    prod = torch.empty((K, C * S, N), dtype=torch.complex64, device="cuda")
    ys = torch.empty_like(prod)
    plain = torch.empty((C, K, L), dtype=torch.complex64, device="cuda")
    out_bytes = C * K * L * 8
    pw = ctypes.c_void_p()
    # the placement search judges its candidates by copies from a read buffer of at least out_bytes: the unfused pipeline's inverse
    # output (5.7 GB) serves
    assert sm.lib.smfft_malloc_written_for(ys.data_ptr(), out_bytes, ctypes.byref(pw)) == 0
    placed = as_tensor(pw.value, (C, K, L))
    info = sm.last_pair_info()
    print(f"smfft_malloc_written_for: {info['mixed_bytes'] / 2**30:.2f} GiB mixed, {info['interleaved_bytes'] / 2**30:.2f} GiB interleaved, "
          f"good_enough={info['good_enough']}, search {info['search_ms']:.0f} ms", flush=True)
    xpad = torch.zeros((C, (S - 1) * V + N), dtype=torch.complex64, device="cuda")
    xpad[:, M - 1:M - 1 + L] = x

    def fused(out):
        return lambda: sm.fir_launch(x.data_ptr(), L, C, H.data_ptr(), K, M, N, out.data_ptr(), "convolve", stream=sp)

    def unfused(out):
        def run():
            frames.view(C, S, N).copy_(xpad.unfold(1, N, V))                 # framing
            sm.launch("ct", "external", frames.data_ptr(), spec.data_ptr(), N, C * S, False, True, stream=sp)
            torch.mul(spec.unsqueeze(0), H.unsqueeze(1), out=prod)            # broadcast multiply by the K spectra (1/N folded in)
            sm.launch("ct", "external", prod.data_ptr(), ys.data_ptr(), N, K * C * S, True, True, stream=sp)
            out.copy_(ys.view(K, C, S, N)[..., M - 1:].reshape(K, C, S * V)[..., :L].permute(1, 0, 2))   # gather
        return run

    fns = {"fused   (smfft_malloc_written_for output)": fused(placed), "fused   (hipMalloc output)": fused(plain),
           "unfused (smfft_malloc_written_for output)": unfused(placed), "unfused (hipMalloc output)": unfused(plain)}
    # the four compute the same thing; compare the fused result with the unfused one and with numpy on a sampled window
    fns["fused   (hipMalloc output)"]()
    fns["unfused (smfft_malloc_written_for output)"]()
    torch.cuda.synchronize()
    d = (plain - placed).abs().max().item() / placed.abs().max().item()
    n0, W = L - 5000, 5000
    xs = x[0, n0 - (M - 1):].cpu().numpy().astype(np.complex128)
    hk = h[K - 1].cpu().numpy().astype(np.complex128)
    want = np.convolve(xs, hk)[M - 1:M - 1 + W]
    got = plain[0, K - 1, n0:].cpu().numpy()
    print(f"max |fused - unfused| / max |unfused| = {d:.2e};  fused vs np.convolve (last row, last {W}): "
          f"relL2 {np.linalg.norm(got - want) / np.linalg.norm(want):.2e}", flush=True)
    print(f"main configuration: C={C} L=2^24 K={K} M={M} N={N} (V={V}, S={S}), output {out_bytes / 2**30:.0f} GiB, {REPS} reps round robin", flush=True)
    ts = round_robin(fns, REPS, stream)
    med = {name: report(name, v, C, L, K, N, M) for name, v in ts.items()}
    for where in ("smfft_malloc_written_for output", "hipMalloc output"):
        print(f"  speed-up fused over unfused, {where}: {med[f'unfused ({where})'] / med[f'fused   ({where})']:.2f} x", flush=True)
    del frames, spec, prod, ys, xpad, placed, plain
    sm.lib.smfft_free_written(pw.value)
    torch.cuda.empty_cache()

    # ---------------------------------------------------------------- sweep, fused only
    print(f"sweep (fused, hipMalloc output, C={C}, L=2^24, M = N/4 + 1):", flush=True)
    for N in (256, 1024, 4096):
        M = N // 4 + 1
        for K in (1, 8, 32, 128):
            h = torch.from_numpy((rng.standard_normal((K, M)) + 1j * rng.standard_normal((K, M))).astype(np.complex64)).cuda()
            H = torch.empty((K, N), dtype=torch.complex64, device="cuda")
            sm.fir_prepare(h.data_ptr(), H.data_ptr(), M, K, N, "convolve", stream=sp)
            out = torch.empty((C, K, L), dtype=torch.complex64, device="cuda")
            fn = (lambda H=H, K=K, M=M, N=N, out=out:
                  sm.fir_launch(x.data_ptr(), L, C, H.data_ptr(), K, M, N, out.data_ptr(), "convolve", stream=sp))
            v = round_robin({"f": fn}, REPS, stream)["f"]
            report(f"N={N:4d} M={M:4d} K={K:3d}", v, C, L, K, N, M)
            del out, H, h
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

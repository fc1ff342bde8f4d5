"""A/B of the N = 8192 / 16384 single-pass C2C kernels (libsmfft_large.so) at 4 GiB in + 4 GiB out: 65536 FFTs at 8192, 32768 at
16384.  For each N x direction x output placement (a smfft_malloc_pair pair; two plain hipMalloc buffers) it records the kernel's
median ms over >= 20 launches after warm-up, TB/s (read + write bytes) and its fraction of 8 TB/s, its fraction of the same-run copy
ceiling (smfft_copy_launch on the same buffers), torch.fft.fft on device tensors of the same shape, and the N = 4096 external kernel
at the same bytes.  Every row is also checked against numpy on the first and the last FFT of the batch.  (The next-FFT prefetch
form of N = 16384 is not measured: it computed wrong results and is not shipped -- DESIGN.md section 9.)

    python tools/ab_large.py [--reps 30] [--out profiles/r09_large_ab.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TBS = 8.0
BYTES_EACH = 4 << 30


def timed(torch, fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def check(sm, din, dout, n, inverse, what):
    """the first and the last FFT of the batch against numpy (complex128)"""
    nffts = BYTES_EACH // (n * 8)
    for f in (0, nffts - 1):
        x = np.empty(n, np.complex64)
        y = np.empty(n, np.complex64)
        sm.lib.smfft_memcpy_d2h(x.ctypes.data, din + f * n * 8, n * 8)
        sm.lib.smfft_memcpy_d2h(y.ctypes.data, dout + f * n * 8, n * 8)
        want = np.fft.ifft(x.astype(np.complex128)) * n if inverse else np.fft.fft(x.astype(np.complex128))
        err = np.linalg.norm(y - want) / np.linalg.norm(want)
        assert err < 5e-7, f"{what}: FFT {f} relL2 {err:.2e}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_large_ab.txt"))
    args = ap.parse_args()
    assert args.reps >= 20
    import torch
    import smfft_amd as sm
    from smfft_amd import large
    sm.FFT_init()
    lb = large.lib()

    x_host = (np.random.default_rng(0).standard_normal(BYTES_EACH // 4, dtype=np.float32) * 0.5).view(np.complex64)
    lines = [f"# tools/ab_large.py: 4 GiB in + 4 GiB out per launch, median of {args.reps} launches after 5 warm-up; "
             f"TB/s = 8 GiB / time; copy = smfft_copy_launch on the same buffers; 4096 = the N = 4096 external kernel at the same bytes",
             f"{'N':>6} {'dir':>3} {'buffers':>6} {'ms':>8} {'TB/s':>6} {'/8TB/s':>6} {'copy ms':>8} {'/copy':>6} "
             f"{'4096 ms':>8} {'torch ms':>9} {'torch/this':>10}"]
    for placement in ("pair", "plain"):
        if placement == "pair":
            a, b = ctypes.c_void_p(), ctypes.c_void_p()
            assert sm.lib.smfft_malloc_pair(BYTES_EACH, ctypes.byref(a), ctypes.byref(b)) == 0
            din, dout = a.value, b.value
        else:
            din, dout = sm.lib.smfft_malloc(BYTES_EACH), sm.lib.smfft_malloc(BYTES_EACH)
        assert din and dout
        assert sm.lib.smfft_memcpy_h2d(din, x_host.ctypes.data, BYTES_EACH) == 0
        copy_ms = timed(torch, lambda: sm.lib.smfft_copy_launch(din, dout, BYTES_EACH // 8, None), args.reps)
        for n in (8192, 16384):
            nffts = BYTES_EACH // (n * 8)
            t_in = torch.from_numpy(x_host[: nffts * n].reshape(nffts, n)).cuda()
            torch_ms = timed(torch, lambda: torch.fft.fft(t_in, dim=-1), args.reps)
            del t_in
            torch.cuda.empty_cache()
            for inverse in (0, 1):
                ext_ms = timed(torch, lambda: sm.lib.smfft_launch(0, 0, din, dout, 4096, BYTES_EACH // (4096 * 8), inverse, 1, None), args.reps)
                assert lb.smfft_large_launch(din, dout, n, nffts, inverse, None) == 0
                torch.cuda.synchronize()
                check(sm, din, dout, n, inverse, f"N={n} inverse={inverse} {placement}")
                ms = timed(torch, lambda: lb.smfft_large_launch(din, dout, n, nffts, inverse, None), args.reps)
                tbs = 2 * BYTES_EACH / (ms * 1e-3) / 1e12
                lines.append(f"{n:>6} {'inv' if inverse else 'fwd':>3} {placement:>6} {ms:8.3f} {tbs:6.2f} {tbs / PEAK_TBS:6.3f} "
                             f"{copy_ms:8.3f} {copy_ms / ms:6.3f} {ext_ms:8.3f} {torch_ms:9.3f} {torch_ms / ms:10.2f}")
                print(lines[-1], flush=True)
        if placement == "pair":
            sm.lib.smfft_free_pair(ctypes.c_void_p(din))
        else:
            sm.lib.smfft_free(din)
            sm.lib.smfft_free(dout)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

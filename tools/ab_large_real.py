"""A/B of the real N = 16384 / 32768 single-pass R2C / C2R kernels (libsmfft_large_real.so) at 4 GiB in + 4 GiB out: 65536 FFTs at
16384, 32768 at 32768.  For each N x direction x output placement (a smfft_malloc_pair pair; two plain hipMalloc buffers) it records
the kernel's median ms over >= 20 launches after warm-up, TB/s (read + write bytes) and its fraction of the same-run copy ceiling
(smfft_copy_launch on the same buffers), smfft_large_launch of the complex length L = N/2 on the same bytes (the C2C the real
transform is built on), and torch.fft.rfft / irfft on device tensors of the same batch.  Every row is also checked against numpy on
the first and the last FFT of the batch.

    python tools/ab_large_real.py [--reps 30] [--out profiles/r10_large_real_ab.txt]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/ab_large_real.py --trace
                                 # --trace: only 10 launches of every real kernel and of the C2C of L on one pair (kernel times)
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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
    """the first and the last FFT of the batch against numpy (float64 / complex128)"""
    from oracle import np_reference as ref
    nffts = BYTES_EACH // (n * 4)
    for f in (0, nffts - 1):
        x = np.empty(n // 2 if inverse else n, np.complex64 if inverse else np.float32)
        y = np.empty(n if inverse else n // 2, np.float32 if inverse else np.complex64)
        sm.lib.smfft_memcpy_d2h(x.ctypes.data, din + f * n * 4, n * 4)
        sm.lib.smfft_memcpy_d2h(y.ctypes.data, dout + f * n * 4, n * 4)
        want = (ref.c2r_packed if inverse else ref.r2c_packed)(x[None])[0]
        err = np.linalg.norm(y - want) / np.linalg.norm(want)
        assert err < 5e-7, f"{what}: FFT {f} relL2 {err:.2e}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_large_real_ab.txt"))
    ap.add_argument("--trace", action="store_true", help="only launch every kernel 10 times on one pair (for rocprofv3)")
    args = ap.parse_args()
    assert args.reps >= 20
    import torch                      # first: torch initialises the HIP runtime before the libraries use it
    import smfft_amd as sm
    from smfft_amd import large, large_real
    sm.FFT_init()
    lb, rb = large.lib(), large_real.lib()
    if args.trace:
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        assert sm.lib.smfft_malloc_pair(BYTES_EACH, ctypes.byref(a), ctypes.byref(b)) == 0
        assert sm.lib.smfft_memset(a.value, 0, BYTES_EACH) == 0
        for n in (16384, 32768):
            nffts = BYTES_EACH // (n * 4)
            for inverse in (0, 1):
                for _ in range(10):
                    assert rb.smfft_large_real_launch(a.value, b.value, n, nffts, inverse, None) == 0
                    assert lb.smfft_large_launch(a.value, b.value, n // 2, nffts, inverse, None) == 0
        assert sm.lib.smfft_synchronize() == 0
        sm.lib.smfft_free_pair(a)
        return

    rng = np.random.default_rng(0)
    x_host = (rng.standard_normal(BYTES_EACH // 4, dtype=np.float32) * 0.5)
    lines = [f"# tools/ab_large_real.py: 4 GiB in + 4 GiB out per launch, median of {args.reps} launches after 5 warm-up; "
             f"TB/s = 8 GiB / time; copy = smfft_copy_launch on the same buffers; C2C(L) = smfft_large_launch of L = N/2 on the same "
             f"buffers; torch = torch.fft.rfft (fwd) / irfft (inv) of the same batch on device tensors",
             f"{'N':>6} {'dir':>3} {'buffers':>6} {'ms':>8} {'TB/s':>6} {'copy ms':>8} {'/copy':>6} "
             f"{'C2C(L) ms':>9} {'this/C2C':>8} {'torch ms':>9} {'torch/this':>10}"]
    for placement in ("pair", "plain"):
        if placement == "pair":
            a, b = ctypes.c_void_p(), ctypes.c_void_p()
            assert sm.lib.smfft_malloc_pair(BYTES_EACH, ctypes.byref(a), ctypes.byref(b)) == 0
            din, dout = a.value, b.value
        else:
            din, dout = sm.lib.smfft_malloc(BYTES_EACH), sm.lib.smfft_malloc(BYTES_EACH)
        assert din and dout
        copy_ms = timed(torch, lambda: sm.lib.smfft_copy_launch(din, dout, BYTES_EACH // 8, None), args.reps)
        for n in (16384, 32768):
            nffts = BYTES_EACH // (n * 4)
            # torch on device tensors of the same batch (allocated after the pair, as tools/ab_large.py does)
            t_x = torch.from_numpy(x_host[: nffts * n].reshape(nffts, n)).cuda()
            torch_ms = [timed(torch, lambda: torch.fft.rfft(t_x, dim=-1), args.reps)]
            t_s = torch.fft.rfft(t_x, dim=-1)
            del t_x
            torch.cuda.empty_cache()
            torch_ms.append(timed(torch, lambda: torch.fft.irfft(t_s, n=n, dim=-1), args.reps))
            del t_s
            torch.cuda.empty_cache()
            for inverse in (0, 1):
                # the input: real samples (R2C) or the packed spectra of them (C2R), made on the device
                assert sm.lib.smfft_memcpy_h2d(din, x_host.ctypes.data, BYTES_EACH) == 0
                if inverse:
                    assert rb.smfft_large_real_launch(din, din, n, nffts, 0, None) == 0
                    torch.cuda.synchronize()
                c2c_ms = timed(torch, lambda: lb.smfft_large_launch(din, dout, n // 2, nffts, inverse, None), args.reps)
                assert rb.smfft_large_real_launch(din, dout, n, nffts, inverse, None) == 0
                torch.cuda.synchronize()
                check(sm, din, dout, n, inverse, f"N={n} inverse={inverse} {placement}")
                ms = timed(torch, lambda: rb.smfft_large_real_launch(din, dout, n, nffts, inverse, None), args.reps)
                tbs = 2 * BYTES_EACH / (ms * 1e-3) / 1e12
                t = torch_ms[inverse]
                lines.append(f"{n:>6} {'inv' if inverse else 'fwd':>3} {placement:>6} {ms:8.3f} {tbs:6.2f} "
                             f"{copy_ms:8.3f} {copy_ms / ms:6.3f} {c2c_ms:9.3f} {ms / c2c_ms:8.3f} {t:9.3f} {t / ms:10.2f}")
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

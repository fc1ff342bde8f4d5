"""The DIF transform against its natural-order neighbours on the config-2 pair (N = 1024, 524 288 series, 4 GiB in and 4 GiB out; one
smfft_malloc_pair), in one process, timed round robin so that drift of the box hits all alike:
  external:     SMFFT_DIF_external<FFT_1024_forward_noreorder> (smfft_ct_dif_launch) | SMFFT_DIT_external<FFT_1024_forward> (smfft_launch)
  convolution:  the reference-contract user kernels of examples/reference_shape_kernel.hip (shared-memory form, register form), the Engine
                form of examples/fft_convolution.hip, and the DIF chain of examples/dif_convolution.hip (DIF -> .* Hb -> no-reorder DIT)
    python tools/ab_dif.py [reps=13]
Prints median / min ms per kernel and the rate of input + output against 8 TB/s."""
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import smfft_amd as sm  # noqa: E402

N, NS = 1024, 524288
BYTES = NS * N * 8
vp, ci = ctypes.c_void_p, ctypes.c_int
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 13


def main():
    sm.FFT_init()
    ex = ctypes.CDLL(os.path.join(os.path.dirname(sm.LIB_PATH), "libsmfft_examples.so"))
    pa, pb = ctypes.c_void_p(), ctypes.c_void_p()
    assert sm.lib.smfft_malloc_pair(BYTES, ctypes.byref(pa), ctypes.byref(pb)) == 0
    chunk = np.random.default_rng(0).random(1 << 22, dtype=np.float32) - 0.5
    sm.lib.smfft_memcpy_h2d(pa.value, chunk.ctypes.data, chunk.nbytes)
    filled = chunk.nbytes
    while filled < BYTES:
        step = min(filled, BYTES - filled)
        sm.lib.smfft_memcpy_d2d(pa.value + filled, pa.value, step)
        filled += step
    h = np.zeros((1, N), np.complex64)
    h[0, :5] = [0.4, 0.3, 0.2, 0.1, -0.05j]
    H = sm.DeviceBuffer.from_host(np.fft.fft(h[0].astype(np.complex128)).astype(np.complex64))
    Hb = sm.DeviceBuffer.from_host(sm.c2c_dif(h)[0])
    for name in ("smfft_example_reference_shape_convolve_1024", "smfft_example_reference_shape_convolve_1024_registers", "smfft_example_convolve_1024_registers"):
        getattr(ex, name).argtypes = [vp, vp, vp, ci, vp]
    ex.smfft_example_reference_shape_convolve_dif.argtypes = [vp, vp, vp, ci, ci, vp]
    groups = {
        "external": {
            "DIF_external<1024 fwd>": lambda: sm.launch_dif(pa.value, pb.value, N, NS),
            "DIT_external<1024 fwd>": lambda: sm.launch("ct", "external", pa.value, pb.value, N, NS, False, True),
        },
        "convolution": {
            "contract shared-memory": lambda: ex.smfft_example_reference_shape_convolve_1024(pa.value, H.ptr, pb.value, NS, None),
            "contract registers": lambda: ex.smfft_example_reference_shape_convolve_1024_registers(pa.value, H.ptr, pb.value, NS, None),
            "Engine registers": lambda: ex.smfft_example_convolve_1024_registers(pa.value, H.ptr, pb.value, NS, None),
            "contract DIF chain": lambda: ex.smfft_example_reference_shape_convolve_dif(pa.value, Hb.ptr, pb.value, N, NS, None),
        },
    }
    # the four convolutions compute the same thing: compare the tails of their outputs
    tail = np.empty(1 << 20, np.float32)
    first = None
    for name, fn in groups["convolution"].items():
        assert fn() in (0, None)
        assert sm.lib.smfft_synchronize() == 0
        sm.lib.smfft_memcpy_d2h(tail.ctypes.data, pb.value + BYTES - tail.nbytes, tail.nbytes)
        if first is None:
            first = tail.copy()
        else:
            print(f"{name:24s} max |difference to the shared-memory form| = {float(np.max(np.abs(tail - first))):.3g}", flush=True)
    for group, fns in groups.items():
        ts = {n: [] for n in fns}
        for rep in range(REPS):
            for name, fn in fns.items():
                if rep == 0:
                    fn(), fn()
                    sm.lib.smfft_synchronize()
                t0 = time.perf_counter()
                fn()
                sm.lib.smfft_synchronize()
                ts[name].append((time.perf_counter() - t0) * 1e3)
        for name in fns:
            v = sorted(ts[name])
            med = v[len(v) // 2]
            print(f"{group:12s} {name:24s} median {med:.3f} ms  min {v[0]:.3f}  ({2 * BYTES / med / 1e9:.2f} TB/s in + out = {2 * BYTES / med / 1e9 / 8:.3f} of 8 TB/s)", flush=True)
    H.free()
    Hb.free()
    sm.lib.smfft_free_pair(pa.value)


if __name__ == "__main__":
    main()

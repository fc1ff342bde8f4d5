"""Every __global__ kernel that libsmfft_large.so ships (N = 8192 / 16384 single-pass C2C, include/smfft_large.h), with the public call
that reaches it and the GPU tests that compare it with fp64, run it on guarded buffers and probe it per element and in isolation
(tests/test_large_cpu.py checks this list against the built library's kernels, with the rule of tests/test_kernel_inventory.py).
Names are the demangled kernel names without their parameter lists."""

LARGE = "tests/test_large_gpu.py::"
_TESTS = [LARGE + "test_large_parity", LARGE + "test_large_round_trip"]
_BOUNDS = [LARGE + "test_large_guarded_buffers_and_interior_pointers", LARGE + "test_large_in_place"]
_PROBES = [LARGE + "test_large_dft_matrix_probe", LARGE + "test_large_zero_mean_accuracy", LARGE + "test_large_isolation_and_exact_scaling"]

KERNELS = {
    f"smfft::large::large_c2c<{n}, {d}>": {
        "call": f"smfft_large_launch / smfft_large_benchmark(FFT_size={n}, inverse={d})",
        "tests": _TESTS,
        "bounds": _BOUNDS,
        "probes": _PROBES,
    }
    for n in (8192, 16384) for d in (0, 1)
}

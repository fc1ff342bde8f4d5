"""Every __global__ kernel that libsmfft_large_real.so ships (real N = 16384 / 32768 single-pass R2C / C2R, include/smfft_large_real.h),
with the public call that reaches it and the GPU tests that compare it with fp64, run it on guarded buffers and probe it per element
and in isolation, and the CPU tests that run it on the host ("host").  tests/test_large_real_cpu.py checks this list against the built
library's kernels, with the rule of tests/test_kernel_inventory.py.  Names are the demangled kernel names without their parameter lists; N is the real length."""

from tests.large_inventory import HOST_TESTS      # the host run of the kernel (tests/hostsim), shared with the C2C kernels

REAL = "tests/test_large_real_gpu.py::"
_TESTS = [REAL + "test_large_real_parity", REAL + "test_large_real_round_trip", REAL + "test_large_real_caller_stream_ordering",
          REAL + "test_large_real_concurrent_streams", REAL + "test_large_real_benchmark_accumulates_and_rejects"]
_BOUNDS = [REAL + "test_large_real_guarded_buffers_and_interior_pointers", REAL + "test_large_real_in_place",
           REAL + "test_large_real_guarded_batches_and_offsets", REAL + "test_large_real_64bit_offsets"]
_PROBES = {0: [REAL + "test_large_real_dft_matrix_probe_r2c", REAL + "test_large_real_constant_and_alternating_inputs"],
           1: [REAL + "test_large_real_dft_matrix_probe_c2r"]}
_ISOLATION = [REAL + "test_large_real_zero_mean_accuracy", REAL + "test_large_real_isolation_and_exact_scaling",
              REAL + "test_large_real_position_invariance"]

KERNELS = {
    f"smfft::large::{name}<{n}>": {
        "call": f"smfft_large_real_launch / smfft_large_real_benchmark(FFT_size={n}, inverse={d})",
        "tests": _TESTS,
        "bounds": _BOUNDS,
        "probes": _PROBES[d] + _ISOLATION,
        "host": HOST_TESTS,
    }
    for n in (16384, 32768) for d, name in ((0, "large_r2c"), (1, "large_c2r"))
}

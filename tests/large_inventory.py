"""Every __global__ kernel that libsmfft_large.so ships (N = 8192 / 16384 single-pass C2C, include/smfft_large.h), with the public call
that reaches it and the GPU tests that compare it with fp64, run it on guarded buffers and probe it per element and in isolation
(the `large` cases of tests/test_probes_gpu.py among them), and the CPU tests that run it on the host and knock its barriers out
("host": tests/test_large_hostsim.py).  tests/test_large_cpu.py checks this list against the built library's kernels, with the rule
of tests/test_kernel_inventory.py; the "host" tests must exist and must NOT need a GPU.
Names are the demangled kernel names without their parameter lists."""

LARGE = "tests/test_large_gpu.py::"
PROBE_SUITE = "tests/test_probes_gpu.py::"
_TESTS = [LARGE + "test_large_parity", LARGE + "test_large_round_trip", LARGE + "test_large_concurrent_streams_and_co_residency"]
_BOUNDS = [LARGE + "test_large_guarded_buffers_and_interior_pointers", LARGE + "test_large_in_place",
           LARGE + "test_large_guarded_batches_and_offsets", LARGE + "test_large_64bit_offsets_8192"]
_PROBES = [LARGE + "test_large_dft_matrix_probe", LARGE + "test_large_zero_mean_accuracy", LARGE + "test_large_isolation_and_exact_scaling",
           LARGE + "test_large_position_invariance",
           PROBE_SUITE + "test_dft_matrix_probe", PROBE_SUITE + "test_zero_mean_accuracy", PROBE_SUITE + "test_isolation_and_exact_scaling"]

# the host run of the kernel (tests/hostsim): the header's own code thread by thread under chosen schedules, with its barriers knocked out
HOST = "tests/test_large_hostsim.py::"
HOST_TESTS = [HOST + "test_host_matches_fp64", HOST + "test_host_dft_matrix_probe", HOST + "test_host_schedule_invariance",
              HOST + "test_host_persistent_loop", HOST + "test_host_guarded_buffers", HOST + "test_host_barrier_knock_out"]

KERNELS = {
    f"smfft::large::large_c2c<{n}, {d}>": {
        "call": f"smfft_large_launch / smfft_large_benchmark(FFT_size={n}, inverse={d})",
        "tests": _TESTS,
        "bounds": _BOUNDS,
        "probes": _PROBES,
        "host": HOST_TESTS,
    }
    for n in (8192, 16384) for d in (0, 1)
}

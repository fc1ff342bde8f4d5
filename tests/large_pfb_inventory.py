"""Every __global__ kernel that libsmfft_large_pfb.so ships (the polyphase filter bank channelizer of include/smfft_large_pfb.h: N = 8192
and 16384 channels, complex and power output), with the public call that reaches it, the GPU tests that compare it with fp64 ("tests")
and run it on guarded buffers, at interior pointers and beyond 2^31 elements ("bounds"), and the run of the kernel on the host
(tests/hostsim: "host").  tests/test_large_pfb_cpu.py checks this list against the built library's kernels, with the rule of
tests/test_kernel_inventory.py.  Names are the demangled kernel names without their parameter lists; the third template argument is the
signal-load policy of the build (0: plain).

"probes": the per-element tap-matrix probe of the small banks (tests/test_pfb_probes_gpu.py) has no counterpart for this bank yet.  What
isolates a pair from its batch here is listed in its place: the bits of a pair do not depend on the schedule, the grid, or the streams
launched with it."""

GPU = "tests/test_large_pfb_gpu.py::"
HOST = "tests/test_large_pfb_hostsim.py::"
SIZES = (8192, 16384)

KERNELS = {
    f"smfft::large::pfb_large<{n}, {power}, 0>": {
        "call": f"smfft_large_pfb_launch / smfft_large_pfb_launch_tuned / smfft_large_pfb_benchmark(n_channels={n}, power={power})",
        "tests": [GPU + t for t in ("test_filter_bank_matches_the_model", "test_multi_round_through_launch_tuned", "test_full_grid")]
        + ([GPU + "test_one_tap_of_ones_is_a_bare_transform"] if not power else []),
        "bounds": [GPU + t for t in ("test_filter_bank_matches_the_model", "test_interior_pointers")]
        + ([GPU + "test_offsets_beyond_two_to_the_31"] if (n, power) == (16384, 0) else []),
        "probes": [GPU + t for t in ("test_every_schedule_and_grid_gives_the_same_bits", "test_three_streams_equal_three_launches")],
        "host": [HOST + t for t in ("test_host_filter_bank_matches_fp64", "test_host_two_streams_equal_two_launches")]
        + ([HOST + t for t in ("test_host_schedule_invariance", "test_host_barrier_knock_out")] if not power else []),
    }
    for n in SIZES for power in (0, 1)
}

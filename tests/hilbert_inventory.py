"""Every __global__ kernel that libsmfft_hilbert.so ships (batched Hilbert transform, analytic signal and envelope of real rows of
include/smfft_hilbert.h: one kernel per kind -- 0 quadrature, 1 analytic, 2 envelope -- and inner transform length M = n / 2 =
256 ... 4096), with the public call that reaches it and the GPU tests that compare it with fp64 ("tests"), run it on guarded buffers,
in place and beyond 2^31 elements ("bounds") and probe it per element and in isolation ("probes").  tests/test_sm_hilbert_cpu.py checks
this list against the built library's kernels, with the rule of tests/test_kernel_inventory.py.  Names are the demangled kernel names
without their parameter lists.

There is no "host" kind here, for the reason tests/dct_inventory.py gives: the kernels' transforms are smfft::Engine<M, DIR, 1>, whose
exchanges at M <= 4096 go through DPP / permlane lane operations; tests/hostsim emulates LDS, barriers and the schedule of a workgroup,
not those cross-lane instructions."""

SIZES = (256, 512, 1024, 2048, 4096)
KINDS = (0, 1, 2)
GPU = "tests/test_sm_hilbert_gpu.py::"


def _entry(m, kind):
    n = 2 * m
    return {
        "call": f"smfft_hilbert_launch / smfft_hilbert_launch_tuned / smfft_hilbert_benchmark(n = {n}, kind = {kind})",
        "tests": [GPU + "test_against_fp64"] + ([GPU + "test_grid_stride_loop"] if m == 256 and kind in (0, 1) else []),
        "bounds": ([GPU + "test_bounds"] if m in (256, 4096) else [GPU + "test_position_grid_and_in_place_are_invisible"])
                  + ([GPU + "test_offsets_beyond_two_to_the_31"] if m == 4096 and kind == 0 else []),
        "probes": [GPU + "test_probe_rows_are_isolated", GPU + "test_position_grid_and_in_place_are_invisible"]
                  + ([GPU + "test_probe_tones_and_impulses"] if m in (256, 2048) else []),
    }


KERNELS = {f"smfft::hilbert::hilbert_kernel<{m}, {kind}>": _entry(m, kind) for m in SIZES for kind in KINDS}

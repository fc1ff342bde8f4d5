"""Every __global__ kernel that libsmfft_bluestein.so ships (batched C2C FFTs of any length 1 ... 2048 of include/smfft_bluestein.h:
one kernel per inner transform length M = 256 ... 4096), with the public call that reaches it and the GPU tests that compare it with
fp64 ("tests"), run it on guarded buffers, at offset bases, in place and beyond 2^31 elements ("bounds") and probe it per output and in
isolation ("probes").  tests/test_sm_bluestein_cpu.py checks this list against the built library's kernels, with the rule of
tests/test_kernel_inventory.py.  Names are the demangled kernel names without their parameter lists.

There is no "host" kind here, for the reason tests/fir_real_inventory.py gives: the kernels' transforms are smfft::Engine<M, DIR, 1>,
whose exchanges at M <= 4096 go through DPP / permlane lane operations; tests/hostsim emulates LDS, barriers and the schedule of a
workgroup, not those cross-lane instructions."""

SIZES = (256, 512, 1024, 2048, 4096)
GPU = "tests/test_sm_bluestein_gpu.py::"
# the lengths n that use M: (smallest, largest)
LENGTHS = {256: (1, 128), 512: (129, 256), 1024: (257, 512), 2048: (513, 1024), 4096: (1025, 2048)}


def _entry(m):
    ends = m in (256, 4096)
    return {
        "call": f"smfft_bluestein_launch / smfft_bluestein_launch_tuned / smfft_bluestein_benchmark(n = {LENGTHS[m][0]} ... {LENGTHS[m][1]})",
        "tests": [GPU + "test_against_fp64", GPU + "test_grid_is_invisible"] + ([GPU + "test_grid_stride_loop"] if ends else []),
        "bounds": ([GPU + "test_bounds"] if ends else [GPU + "test_against_fp64"])
                  + ([GPU + "test_in_place"] if m in (512, 4096) else [])
                  + ([GPU + "test_offsets_beyond_two_to_the_31"] if m == 4096 else []),
        "probes": [GPU + "test_probe_impulses", GPU + "test_probe_tone"] + ([GPU + "test_probe_rows_are_isolated"] if ends else []),
    }


KERNELS = {f"smfft::bluestein::bluestein_kernel<{m}>": _entry(m) for m in SIZES}

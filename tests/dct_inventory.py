"""Every __global__ kernel that libsmfft_dct.so ships (batched DCT / DST of types II and III of real rows of include/smfft_dct.h: the
type II and the type III kernel per inner transform length M = n / 2 = 256 ... 4096), with the public call that reaches it and the GPU
tests that compare it with fp64 ("tests"), run it on guarded buffers, in place and beyond 2^31 elements ("bounds") and probe it per
element and in isolation ("probes").  tests/test_sm_dct_cpu.py checks this list against the built library's kernels, with the rule of
tests/test_kernel_inventory.py.  Names are the demangled kernel names without their parameter lists.

There is no "host" kind here, for the reason tests/rowconv_real_inventory.py gives: the kernels' transforms are
smfft::Engine<M, DIR, 1>, whose exchanges at M <= 4096 go through DPP / permlane lane operations; tests/hostsim emulates LDS, barriers
and the schedule of a workgroup, not those cross-lane instructions."""

SIZES = (256, 512, 1024, 2048, 4096)
GPU = "tests/test_sm_dct_gpu.py::"


def _entry(m, type):
    n = 2 * m
    return {
        "call": f"smfft_dct_launch / smfft_dct_launch_tuned / smfft_dct_benchmark(n = {n}, type = {type})",
        "tests": [GPU + "test_against_fp64", GPU + "test_round_trip"] + ([GPU + "test_grid_stride_loop"] if m == 256 else []),
        "bounds": ([GPU + "test_bounds"] if m in (256, 4096) else [GPU + "test_position_grid_and_in_place_are_invisible"])
                  + ([GPU + "test_offsets_beyond_two_to_the_31"] if m == 4096 else []),
        "probes": [GPU + "test_probe_rows_are_isolated", GPU + "test_position_grid_and_in_place_are_invisible"]
                  + ([GPU + "test_probe_impulses"] if m in (256, 2048) else []),
    }


KERNELS = {f"smfft::dct::dct{type}_kernel<{m}>": _entry(m, type) for m in SIZES for type in (2, 3)}

"""Every __global__ kernel that libsmfft_rowconv_real.so ships (batched convolution / correlation of pairs of real rows of
include/smfft_rowconv_real.h: one kernel per inner transform length M = 256 ... 4096), with the public call that reaches it and the GPU
tests that compare it with fp64 ("tests"), run it on guarded buffers, at offset bases, through windows and beyond 2^31 elements
("bounds") and probe it per output and in isolation ("probes").  tests/test_sm_rowconv_real_cpu.py checks this list against the built
library's kernels, with the rule of tests/test_kernel_inventory.py.  Names are the demangled kernel names without their parameter
lists.

There is no "host" kind here, for the reason tests/fir_real_inventory.py gives: the kernels' transforms are smfft::Engine<M, DIR, 1>,
whose exchanges at M <= 4096 go through DPP / permlane lane operations, and the row reductions of this kernel are ds_bpermute
butterflies; tests/hostsim emulates LDS, barriers and the schedule of a workgroup, not those cross-lane instructions."""

SIZES = (256, 512, 1024, 2048, 4096)
GPU = "tests/test_sm_rowconv_real_gpu.py::"
# shapes (n_a, n_b) of the GPU tests that use M: n_a + n_b - 1 in (M / 2, M], or <= 256
SHAPES = {256: ((1, 1), (1, 256), (256, 1), (128, 129), (5, 3)), 512: ((129, 129), (300, 200), (200, 300), (256, 257)),
          1024: ((1000, 25), (512, 513)), 2048: ((1000, 26), (1536, 513), (1025, 1024), (1024, 1025)),
          4096: ((4095, 2), (2, 4095), (4096, 1), (1, 4096), (2048, 2049), (2048, 2048))}


def _entry(m):
    return {
        "call": f"smfft_rowconv_real_launch / smfft_rowconv_real_launch_tuned / smfft_rowconv_real_benchmark(n_a + n_b - 1 {'<=' if m == 256 else f'in {m // 2 + 1} ...'} {m})",
        "tests": [GPU + "test_against_fp64", GPU + "test_grid_is_invisible"] + ([GPU + "test_grid_stride_loop"] if m in (256, 2048) else [])
                 + ([GPU + "test_scales"] if m in (512, 4096) else []),
        "bounds": ([GPU + "test_bounds", GPU + "test_window"] if m in (512, 4096) else [GPU + "test_against_fp64"])
                  + ([GPU + "test_offsets_beyond_two_to_the_31"] if m == 4096 else []),
        "probes": [GPU + "test_probe_impulses"]
                  + ([GPU + "test_probe_autocorrelation"] if m in (512, 4096) else [])
                  + ([GPU + "test_probe_rows_are_isolated"] if m in (256, 512, 4096) else [])
                  + ([GPU + "test_row_bits_do_not_depend_on_position"] if m in (256, 1024, 4096) else []),
    }


KERNELS = {f"smfft::rowconv_real::rowconv_real_kernel<{m}>": _entry(m) for m in SIZES}

"""Every __global__ kernel that libsmfft_mdct.so ships (batched DCT-IV / DST-IV of real rows and the MDCT / IMDCT of
include/smfft_mdct.h: dct4_kernel, mdct_kernel and imdct_kernel per inner transform length M = n / 2 = 256 ... 4096), with the public
call that reaches it and the GPU tests that compare it with fp64 ("tests"), run it on guarded buffers, in place and beyond 2^31 elements
("bounds") and probe it per element and in isolation ("probes").  tests/test_sm_mdct_cpu.py checks this list against the built
library's kernels, with the rule of tests/test_kernel_inventory.py.  Names are the demangled kernel names without their parameter lists.

There is no "host" kind here, for the reason tests/rowconv_real_inventory.py gives: the kernels' transforms are
smfft::Engine<M, 0, 1>, whose exchanges at M <= 4096 go through DPP / permlane lane operations; tests/hostsim emulates LDS, barriers
and the schedule of a workgroup, not those cross-lane instructions."""

SIZES = (256, 512, 1024, 2048, 4096)
FAMILIES = ("dct4", "mdct", "imdct")
GPU = "tests/test_sm_mdct_gpu.py::"


def _entry(m, family):
    n = 2 * m
    call = {"dct4": "smfft_dct4_launch / smfft_dct4_launch_tuned / smfft_dct4_benchmark",
            "mdct": "smfft_mdct_launch / smfft_mdct_launch_tuned / smfft_mdct_benchmark",
            "imdct": "smfft_imdct_launch / smfft_imdct_launch_tuned / smfft_imdct_benchmark"}[family]
    return {
        "call": f"{call}({'n' if family == 'dct4' else 'N'} = {n})",
        "tests": [GPU + "test_against_fp64"] + ([GPU + "test_involution"] if family == "dct4" else [])
                 + ([GPU + "test_lapped_transform_reconstructs_the_signal"] if family != "dct4" and m in (256, 4096) else [])
                 + ([GPU + "test_grid_stride_loop"] if m == 256 else []),
        "bounds": ([GPU + "test_bounds"] if m in (256, 4096) else [GPU + "test_position_grid_and_in_place_are_invisible"])
                  + ([GPU + "test_offsets_beyond_two_to_the_31"] if m == 4096 and family == "dct4" else []),
        "probes": [GPU + "test_probe_rows_are_isolated", GPU + "test_position_grid_and_in_place_are_invisible"]
                  + ([GPU + "test_probe_impulses"] if m in (256, 4096) else []),
    }


KERNELS = {f"smfft::mdct::{family}_kernel<{m}>": _entry(m, family) for m in SIZES for family in FAMILIES}

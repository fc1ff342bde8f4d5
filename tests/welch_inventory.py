"""Every __global__ kernel that libsmfft_welch.so ships (the Welch power and cross spectra of include/smfft_welch.h: welch_kernel for
the sums of |X|^2 and csd_kernel for the sums of conj(X) Y, per inner transform length M = n / 2 = 256 ... 4096), with the public call
that reaches it and the GPU tests that compare it with fp64 ("tests"), run it on guarded buffers ("bounds") and probe it per group and
in isolation ("probes").  tests/test_sm_welch_cpu.py checks this list against the built library's kernels, with the rule of
tests/test_kernel_inventory.py.  Names are the demangled kernel names without their parameter lists.

There is no "host" kind here, for the reason tests/rowconv_real_inventory.py and tests/stft_inventory.py give: the kernels' transform
is smfft::Engine<M, 0, 1>, whose exchanges at M <= 4096 go through DPP / permlane lane operations; tests/hostsim emulates LDS, barriers
and the schedule of a workgroup, not those cross-lane instructions."""

SIZES = (256, 512, 1024, 2048, 4096)
FAMILIES = ("welch", "csd")
GPU = "tests/test_sm_welch_gpu.py::"


def _entry(m, family):
    n = 2 * m
    return {
        "call": f"smfft_{family}_launch / smfft_{family}_launch_tuned / smfft_{family}_benchmark(n = {n})",
        "tests": [GPU + ("test_auto_against_fp64" if family == "welch" else "test_cross_against_fp64")]
                 + ([GPU + "test_auto_is_the_sequential_sum_of_the_stft_powers"] if family == "welch" else
                    [GPU + "test_cross_of_a_signal_with_itself", GPU + "test_y_stride_zero_is_a_repeated_reference"]),
        "bounds": [GPU + "test_bounds"] if m in (256, 4096) else [GPU + "test_position_grid_and_batch_are_invisible"],
        "probes": [GPU + "test_position_grid_and_batch_are_invisible", GPU + "test_nan_stays_in_its_groups"],
    }


KERNELS = {f"smfft::welch::{family}_kernel<{m}>": _entry(m, family) for m in SIZES for family in FAMILIES}

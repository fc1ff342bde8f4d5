"""Every __global__ kernel that libsmfft_bands.so ships (the band spectrograms of include/smfft_bands.h: bands_kernel, the STFT power
kind's frames summed along frequency into the bands of a prepared table, per inner transform length M = n / 2 = 256 ... 4096), with the
public call that reaches it and the GPU tests that compare it with fp64 and with the STFT library's bits ("tests"), run it on guarded
buffers ("bounds") and probe it per frame and in isolation ("probes").  tests/test_sm_bands_cpu.py checks this list against the built
library's kernels, with the rule of tests/test_kernel_inventory.py.  Names are the demangled kernel names without their parameter lists.

There is no "host" kind here, for the reason tests/rowconv_real_inventory.py, tests/stft_inventory.py and tests/welch_inventory.py
give: the kernels' transform is smfft::Engine<M, 0, 1>, whose exchanges at M <= 4096 go through DPP / permlane lane operations;
tests/hostsim emulates LDS, barriers and the schedule of a workgroup, not those cross-lane instructions."""

SIZES = (256, 512, 1024, 2048, 4096)
GPU = "tests/test_sm_bands_gpu.py::"


def _entry(m):
    n = 2 * m
    return {
        "call": f"smfft_bands_launch / smfft_bands_launch_tuned / smfft_bands_benchmark(n = {n})",
        "tests": [GPU + "test_identity_table_is_the_stft_power", GPU + "test_mel_against_fp64"] + ([GPU + "test_awkward_table"] if m in (256, 4096) else []),
        "bounds": [GPU + "test_bounds"] if m in (256, 4096) else [GPU + "test_position_grid_and_batch_are_invisible"],
        "probes": [GPU + "test_position_grid_and_batch_are_invisible", GPU + "test_nan_stays_in_its_frames"],
    }


KERNELS = {f"smfft::bands::bands_kernel<{m}>": _entry(m) for m in SIZES}

"""Every __global__ kernel that libsmfft_stft.so ships (the short-time Fourier transform of include/smfft_stft.h: stft_kernel for the
complex spectrum and for the power, and istft_kernel, per inner transform length M = n / 2 = 256 ... 4096), with the public call that
reaches it and the GPU tests that compare it with fp64 ("tests"), run it on guarded buffers ("bounds") and probe it per element and in
isolation ("probes").  tests/test_sm_stft_cpu.py checks this list against the built library's kernels, with the rule of
tests/test_kernel_inventory.py.  Names are the demangled kernel names without their parameter lists.

There is no "host" kind here, for the reason tests/rowconv_real_inventory.py gives: the kernels' transforms are
smfft::Engine<M, 0, 1> and smfft::Engine<M, 1, 1>, whose exchanges at M <= 4096 go through DPP / permlane lane operations;
tests/hostsim emulates LDS, barriers and the schedule of a workgroup, not those cross-lane instructions."""

SIZES = (256, 512, 1024, 2048, 4096)
FAMILIES = ("stft", "istft")
GPU = "tests/test_sm_stft_gpu.py::"


def _entry(m, family, kind):
    n = 2 * m
    call = {"stft": "smfft_stft_launch / smfft_stft_launch_tuned / smfft_stft_benchmark",
            "istft": "smfft_istft_launch / smfft_istft_launch_tuned / smfft_istft_benchmark"}[family]
    return {
        "call": f"{call}(n = {n}" + (f", kind = {kind})" if family == "stft" else ")"),
        "tests": [GPU + "test_against_fp64"] + ([GPU + "test_round_trip"] if m in (256, 4096) and kind != 1 else [])
                 + ([GPU + "test_power_is_the_square_of_the_complex_kind"] if family == "stft" else [])
                 + ([GPU + "test_grid_stride_loop"] if m == 256 else []),
        "bounds": [GPU + "test_bounds"] if m in (256, 4096) else [GPU + "test_position_and_grid_are_invisible"],
        "probes": [GPU + "test_probe_rows_are_isolated", GPU + "test_position_and_grid_are_invisible"]
                  + ([GPU + "test_probe_impulses"] if m in (256, 4096) else []),
    }


KERNELS = {f"smfft::stft::stft_kernel<{m}, {kind}>": _entry(m, "stft", kind) for m in SIZES for kind in (0, 1)}
KERNELS.update({f"smfft::stft::istft_kernel<{m}>": _entry(m, "istft", None) for m in SIZES})

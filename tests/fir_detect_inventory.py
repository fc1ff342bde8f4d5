"""Every __global__ kernel that libsmfft_fir_detect.so ships (the detected outputs of the overlap-save FIR filter banks of
include/smfft_fir_detect.h: N = 256 ... 4096), with the public call that reaches it and the GPU tests that compare it with fp64
("tests"), run it on guarded buffers, at offset bases and beyond 2^31 elements ("bounds") and probe it per output and in isolation
("probes").  tests/test_fir_detect_cpu.py checks this list against the built library's kernels, with the rule of
tests/test_kernel_inventory.py.  Names are the demangled kernel names without their parameter lists.

There is no "host" kind here, for the reason tests/fir_real_inventory.py gives: the kernels' transforms are smfft::Engine<N, DIR, 1>,
whose exchanges at N <= 4096 go through DPP / permlane lane operations; tests/hostsim emulates LDS, barriers and the schedule of a
workgroup, not those cross-lane instructions."""

SIZES = (256, 512, 1024, 2048, 4096)
GPU = "tests/test_run_fir_detect_gpu.py::"
PROBES = [GPU + "test_probe_identical_filters", GPU + "test_probe_power_of_two_filters", GPU + "test_probe_nan_sample", GPU + "test_probe_nan_tap"]


def _power(n):
    return {
        "call": f"smfft_fir_power_launch / smfft_fir_power_benchmark(FFT_size={n})",
        "tests": [GPU + "test_power_against_fp64"] + ([GPU + "test_filter_groups"] if n == 1024 else [])
                 + ([GPU + "test_grid_stride_loop"] if n in (256, 4096) else []),
        "bounds": ([GPU + "test_bounds"] if n in (256, 4096) else [GPU + "test_power_against_fp64"])
                  + ([GPU + "test_power_offsets_beyond_two_to_the_31"] if n == 1024 else []),
        "probes": PROBES if n in (256, 4096) else [GPU + "test_peak_equals_the_librarys_own_power"],
    }


def _peak(n):
    return {
        "call": f"smfft_fir_peak_launch / smfft_fir_peak_benchmark(FFT_size={n})",
        "tests": [GPU + "test_peak_against_fp64", GPU + "test_peak_equals_the_librarys_own_power"]
                 + ([GPU + "test_filter_groups"] if n == 1024 else []) + ([GPU + "test_grid_stride_loop"] if n in (256, 4096) else []),
        "bounds": [GPU + "test_bounds"] if n in (256, 4096) else [GPU + "test_peak_against_fp64"],
        "probes": PROBES if n in (256, 4096) else [GPU + "test_peak_equals_the_librarys_own_power"],
    }


KERNELS = {f"smfft::fir_detect::fir_power_kernel<{n}>": _power(n) for n in SIZES}
KERNELS.update({f"smfft::fir_detect::fir_peak_kernel<{n}>": _peak(n) for n in SIZES})

"""Every __global__ kernel that libsmfft_fir_real.so ships (the overlap-save FIR filter banks for real signals and real taps of
include/smfft_fir_real.h: N = 256 ... 4096), with the public call that reaches it and the GPU tests that compare it with fp64 ("tests"),
run it on guarded buffers, at offset bases and beyond 2^31 elements ("bounds") and probe it per output and in isolation ("probes").
tests/test_fir_real_cpu.py checks this list against the built library's kernels, with the rule of tests/test_kernel_inventory.py.  Names
are the demangled kernel names without their parameter lists.

There is no "host" kind here: the kernels' transforms are smfft::Engine<N, DIR, 1>, whose exchanges at N <= 4096 go through DPP /
permlane lane operations; tests/hostsim emulates LDS, barriers and the schedule of a workgroup, not those cross-lane instructions."""

SIZES = (256, 512, 1024, 2048, 4096)
GPU = "tests/test_real_fir_gpu.py::"


def _fir(n):
    return {
        "call": f"smfft_fir_real_launch / smfft_fir_real_benchmark(FFT_size={n})",
        "tests": [GPU + "test_filter_bank_matches_numpy", GPU + "test_grid_stride_loop_with_wrapped_prefetch"],
        "bounds": [GPU + "test_bounds"] + ([GPU + "test_output_offsets_beyond_two_to_the_31"] if n == 1024 else []),
        "probes": [GPU + "test_probe_exact_scaling", GPU + "test_probe_nan_sample", GPU + "test_probe_nan_tap"],
    }


def _prepare(n):
    return {
        "call": f"smfft_fir_real_prepare(FFT_size={n})",
        "tests": [GPU + "test_prepared_spectra"],
        "bounds": [GPU + "test_bounds"],
        "probes": [GPU + "test_probe_nan_tap"],
    }


KERNELS = {f"smfft::fir_real::fir_real_overlap_save_kernel<{n}>": _fir(n) for n in SIZES}
KERNELS.update({f"smfft::fir_real::fir_real_prepare_kernel<{n}>": _prepare(n) for n in SIZES})

"""Every __global__ kernel that libsmfft_pfb_spec.so ships (the integrated power spectra of include/smfft_pfb_spec.h: N = 256 ... 4096,
complex and real streams), with the public call that reaches it and the GPU tests that compare it with fp64 ("tests"), run it on
guarded buffers, at interior pointers and beyond 2^31 elements ("bounds") and probe it per spectrum and in isolation ("probes": the
functions of tests/pfb_spec_probes.py).  tests/test_pfb_spec_cpu.py checks this list against the built library's kernels, with the rule
of tests/test_kernel_inventory.py.  Names are the demangled kernel names without their parameter lists.

There is no "host" kind here, for the reason tests/pfb_inventory.py gives: the kernels' transform is smfft::Engine<N, 0, 1>, which
exchanges through DPP / permlane, and the real bank's register split goes through ds_bpermute; tests/hostsim emulates LDS, barriers and
the schedule of a workgroup, not those cross-lane instructions."""

TEST = "tests/test_pfb_spec_gpu.py::test_integrated_spectra"

SIZES = (256, 512, 1024, 2048, 4096)


def _entry(prefix, n, real):
    """the library has one GPU test, which loops over the lengths and both banks (tests/test_pfb_spec_gpu.py says why); its parts:
    tests   check_integrated_spectra_match_the_model, check_output_is_the_shipped_power_mode_summed_in_frame_order,
            check_every_grid_gives_the_same_bits at every (n, real); check_three_streams_equal_three_launches at n in (512, 2048),
            check_caller_stream at 1024, check_benchmark_adds_to_its_total at 2048
    bounds  every run goes through the guarded run of tests/pfb_gpu_harness.py (a NaN-fenced signal, a prefilled output and a guard
            behind it), so the parity grid is the guarded-buffer run of every kernel; check_interior_pointers at n in (256, 4096); check_offsets_beyond_two_to_the_31 at
            (1024, complex)
    probes  the four probe_* functions of tests/pfb_spec_probes.py at every (n, real)"""
    return {
        "call": f"{prefix}_launch / {prefix}_launch_tuned / {prefix}_benchmark(n_channels={n})",
        "tests": [TEST],
        "bounds": [TEST],
        "probes": [TEST],
    }


KERNELS = {f"smfft::pfb_spec::pfb_spec_kernel<{n}>": _entry("smfft_pfb_spec", n, False) for n in SIZES}
KERNELS.update({f"smfft::pfb_spec::pfb_real_spec_kernel<{n}>": _entry("smfft_pfb_real_spec", n, True) for n in SIZES})

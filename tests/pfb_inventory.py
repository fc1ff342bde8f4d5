"""Every __global__ kernel that libsmfft_pfb.so and libsmfft_pfb_real.so ship (the polyphase filter bank channelizers of
include/smfft_pfb.h and include/smfft_pfb_real.h: N = 256 ... 4096, complex and power output), with the public call that reaches it and
the GPU tests that compare it with fp64 ("tests"), run it on guarded buffers, at interior pointers and beyond 2^31 elements ("bounds")
and probe it per element and in isolation ("probes": tests/test_pfb_probes_gpu.py).  tests/test_pfb_cpu.py and
tests/test_pfb_real_cpu.py check these lists against the built libraries' kernels, with the rule of tests/test_kernel_inventory.py.
Names are the demangled kernel names without their parameter lists.

There is no "host" kind here, unlike tests/large_inventory.py: the kernels cannot run on tests/hostsim.  Their transform is
smfft::Engine<N, 0, 1>, which exchanges through DPP / permlane, and the real bank's register split goes through ds_bpermute; hostsim
emulates LDS, barriers and the schedule of a workgroup, not those cross-lane instructions."""

PFB = "tests/test_pfb_gpu.py::"
REAL = "tests/test_pfb_real_gpu.py::"
PROBES = "tests/test_pfb_probes_gpu.py::"

_PROBES = [PROBES + t for t in ("test_tap_matrix_probe", "test_equal_windows_give_equal_bits", "test_streams_and_taps_scale_exactly",
                                "test_nan_sample_reaches_exactly_its_frames", "test_nan_tap_reaches_every_frame")]
SIZES = (256, 512, 1024, 2048, 4096)

# (test, the (N, power) it runs): the same names in both modules unless said otherwise
_TESTS = [
    ("test_filter_bank_matches_the_model", lambda n, power: True),
    ("test_one_tap_of_ones_is_a_bare_{bare}", lambda n, power: not power),
    ("test_every_schedule_gives_the_same_bits", lambda n, power: (n, power) in ((1024, 0), (4096, 1), (256, 0))),
    ("test_three_streams_equal_three_launches", lambda n, power: n in (512, 2048)),
    ("test_caller_stream", lambda n, power: n == 1024),
    ("test_benchmark_adds_to_its_total", lambda n, power: (n, power) == (2048, 0)),
    ("test_channelize_and_prototype_on_two_tones", lambda n, power: n in (256, 1024, 4096)),
]
# every run of the two modules goes through the guarded run of tests/pfb_gpu_harness.py: a NaN-fenced signal, a prefilled output and a
# guard behind it, so the parity grid is the guarded-buffer test of every kernel
_BOUNDS = [
    ("test_filter_bank_matches_the_model", lambda n, power: True),
    ("test_interior_pointers", lambda n, power: n in (256, 4096)),
]


def _pick(module, table, n, power, bare):
    return [module + name.format(bare=bare) for name, runs in table if runs(n, power)]


KERNELS = {
    f"smfft::pfb::pfb_kernel<{n}, {power}>": {
        "call": f"smfft_pfb_launch / smfft_pfb_launch_tuned / smfft_pfb_benchmark(n_channels={n}, power={power})",
        "tests": _pick(PFB, _TESTS, n, power, "transform"),
        "bounds": _pick(PFB, _BOUNDS, n, power, "") + ([PFB + "test_offsets_beyond_two_to_the_31"] if (n, power) == (1024, 0) else []),
        "probes": _PROBES,
    }
    for n in SIZES for power in (0, 1)
}

REAL_KERNELS = {
    f"smfft::pfb_real::pfb_real_kernel<{n}, {power}>": {
        "call": f"smfft_pfb_real_launch / smfft_pfb_real_launch_tuned / smfft_pfb_real_benchmark(n_channels={n}, power={power})",
        "tests": _pick(REAL, _TESTS, n, power, "r2c")
        + ([REAL + "test_agrees_with_the_complex_bank_of_2n_channels"] if n <= 2048 and not power else []),
        "bounds": _pick(REAL, _BOUNDS, n, power, ""),
        "probes": _PROBES,
    }
    for n in SIZES for power in (0, 1)
}

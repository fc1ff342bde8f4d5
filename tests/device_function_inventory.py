"""Every public function of the header-only device API -- each `__device__ void` and `__global__ void` template at global scope or in
namespace smfft::tiled of include/smfft/smfft_device_functions.hpp and include/smfft/smfft_dif.hpp -- with the parameter classes and
directions that GPU tests compare with fp64, and those tests.  tests/test_device_function_inventory.py reads the functions from the
header text and fails on a function without an entry, an entry without a function, or a named test that does not exist or is not a
GPU test, or an entry without probe tests.  (The `__forceinline__` helpers of namespace smfft are the engine behind these functions, not API.)

FUNCTIONS: qualified name -> {"classes": what is tested, "tests": test ids ("tests/<file>::<function>"; a parametrized test is named
by its function), "probes": the tests that probe it per element, on zero-mean data, against the accuracy ratchet and in isolation
(tests/test_device_probes_gpu.py, over the cases of tests/probe_cases.py HEADER_CASES whose HEADER_FUNCS entry names the function)}."""

PARITY = "tests/test_gpu_parity.py::"
CONTRACT = "tests/test_device_contract_gpu.py::"
DIF = "tests/test_dif_gpu.py::"
PROBES = ["tests/test_device_probes_gpu.py::test_dft_matrix_probe", "tests/test_device_probes_gpu.py::test_zero_mean_accuracy",
          "tests/test_device_probes_gpu.py::test_isolation_and_exact_scaling"]

FUNCTIONS = {
    # ---- the reference's contract, global namespace
    "do_SMFFT_CT_DIT": {
        "classes": "all 32 FFT_<N>_{forward,inverse}{,_noreorder} and the 12 _wave64 classes; fill / call / drain, five header builds; "
                   "in a runtime loop; in SMFFT_DIT_multiple",
        "tests": [PARITY + "test_reference_shaped_kernel_matches_oracle", PARITY + "test_wave64_full_small_length_classes_match_oracle",
                  PARITY + "test_device_function_in_a_runtime_loop", PARITY + "test_reference_shaped_kernel_full_occupancy",
                  CONTRACT + "test_ct_multiple_three_applications"],
        "probes": PROBES,
    },
    "do_SMFFT_CT_DIT_registers": {
        "classes": "the 20 CT classes of N = 256 ... 4096, both directions, natural order and no reorder; four header builds",
        "tests": [CONTRACT + "test_ct_dit_registers", CONTRACT + "test_full_occupancy"],
        "probes": PROBES,
    },
    "do_SMFFT_CT_DIT_registers_out": {
        "classes": "the 20 CT classes of N = 256 ... 4096 through SMFFT_DIT_external (fused build)",
        "tests": [PARITY + "test_reference_shaped_kernel_matches_oracle"],
        "probes": PROBES,
    },
    "do_FFT_Stockham_C2C_registers": {
        "classes": "FFT_32 ... FFT_4096, FFT_forward and FFT_inverse; four header builds",
        "tests": [CONTRACT + "test_stockham_registers", CONTRACT + "test_full_occupancy"],
        "probes": PROBES,
    },
    "do_FFT_Stockham_C2C_registers_out": {
        "classes": "FFT_32 ... FFT_4096, FFT_forward and FFT_inverse; four header builds",
        "tests": [CONTRACT + "test_stockham_registers", CONTRACT + "test_full_occupancy", CONTRACT + "test_fft_gpu_external_small"],
        "probes": PROBES,
    },
    "do_FFT_Stockham_mk6": {
        "classes": "FFT_32 ... FFT_4096 on exactly N float2; four header builds; in FFT_GPU_multiple",
        "tests": [CONTRACT + "test_stockham_fill_call_drain", CONTRACT + "test_full_occupancy",
                  CONTRACT + "test_fft_gpu_multiple_three_applications"],
        "probes": PROBES,
    },
    "do_FFT_Stockham_C2C": {
        "classes": "FFT_32 ... FFT_4096, FFT_forward and FFT_inverse on N + 1 float2; four header builds; forward / inverse chains",
        "tests": [CONTRACT + "test_stockham_fill_call_drain", CONTRACT + "test_full_occupancy", CONTRACT + "test_chain_in_a_runtime_loop"],
        "probes": PROBES,
    },
    "do_FFT_Stockham_R2C_C2R": {
        "classes": "FFT_32 ... FFT_2048 (L = real length / 2 <= 2048), FFT_forward and FFT_inverse on L + 1 float2; four header builds; "
                   "R2C / C2R chains; in FFT_GPU_R2C_C2R_multiple",
        "tests": [CONTRACT + "test_r2c_c2r_fill_call_drain", CONTRACT + "test_full_occupancy", CONTRACT + "test_chain_in_a_runtime_loop",
                  CONTRACT + "test_rc_multiple_three_applications"],
        "probes": PROBES,
    },
    "SMFFT_DIT_external": {
        "classes": "all 32 CT classes and the 12 _wave64 classes; five header builds",
        "tests": [PARITY + "test_reference_shaped_kernel_matches_oracle", PARITY + "test_wave64_full_small_length_classes_match_oracle",
                  PARITY + "test_reference_shaped_kernel_full_occupancy"],
        "probes": PROBES,
    },
    "SMFFT_DIT_multiple": {
        "classes": "all 32 CT classes and the 12 _wave64 classes, NREUSES = 3",
        "tests": [CONTRACT + "test_ct_multiple_three_applications"],
        "probes": PROBES,
    },
    "FFT_GPU_external": {
        "classes": "FFT_32 ... FFT_4096; FFT_32 ... FFT_128 in four header builds",
        "tests": [PARITY + "test_reference_shaped_stockham_kernel", CONTRACT + "test_fft_gpu_external_small"],
        "probes": PROBES,
    },
    "FFT_GPU_multiple": {
        "classes": "FFT_32 ... FFT_4096, NREUSES = 3",
        "tests": [CONTRACT + "test_fft_gpu_multiple_three_applications"],
        "probes": PROBES,
    },
    "FFT_GPU_R2C_C2R_external": {
        "classes": "FFT_256 ... FFT_2048, FFT_forward and FFT_inverse",
        "tests": [PARITY + "test_reference_shaped_r2c_c2r_kernel"],
        "probes": PROBES,
    },
    "FFT_GPU_R2C_C2R_multiple": {
        "classes": "FFT_32 ... FFT_2048, FFT_forward and FFT_inverse, NREUSES = 3",
        "tests": [CONTRACT + "test_rc_multiple_three_applications"],
        "probes": PROBES,
    },
    # ---- decimation in frequency (smfft_dif.hpp)
    "do_SMFFT_CT_DIF": {
        "classes": "FFT_<N>_{forward,inverse}_noreorder, N = 32 ... 4096, and the _wave64 no-reorder classes",
        "tests": [DIF + "test_device_function_dif", DIF + "test_contract_convolution_dif"],
        "probes": PROBES,
    },
    "do_SMFFT_CT_DIF_registers": {
        "classes": "FFT_<N>_{forward,inverse}_noreorder, N = 256 ... 4096",
        "tests": [DIF + "test_device_function_dif", DIF + "test_register_chain_dif_then_no_reorder_dit"],
        "probes": PROBES,
    },
    # ---- the engine's tiled contract (256 threads, 4096 / N transforms per workgroup)
    "smfft::tiled::do_SMFFT_CT_DIT": {
        "classes": "all 32 FFT_<N>_{forward,inverse}{,_noreorder}, N = 32 ... 4096, at a stride of 17 N / 16; four header builds; "
                   "FFT_1024_forward / FFT_1024_inverse and FFT_256_* in the convolution example",
        "tests": [CONTRACT + "test_tiled_ct_dit", PARITY + "test_example_convolution_kernel"],
        "probes": PROBES,
    },
    "smfft::tiled::do_FFT_Stockham_mk6": {
        "classes": "FFT_32 ... FFT_4096 at a stride of 17 N / 16; four header builds",
        "tests": [CONTRACT + "test_tiled_stockham_and_r2c"],
        "probes": PROBES,
    },
    "smfft::tiled::do_FFT_Stockham_C2C": {
        "classes": "FFT_32 ... FFT_4096, FFT_forward and FFT_inverse, stride 17 N / 16; four header builds",
        "tests": [CONTRACT + "test_tiled_stockham_and_r2c", CONTRACT + "test_full_occupancy"],
        "probes": PROBES,
    },
    "smfft::tiled::do_FFT_Stockham_R2C_C2R": {
        "classes": "FFT_32 ... FFT_2048, FFT_forward and FFT_inverse, stride 17 N / 16; four header builds",
        "tests": [CONTRACT + "test_tiled_stockham_and_r2c", CONTRACT + "test_full_occupancy"],
        "probes": PROBES,
    },
}

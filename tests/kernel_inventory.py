"""Every __global__ kernel that libsmfft_amd.so ships, with the public call that reaches it and the GPU tests that compare it with an fp64
reference (tests/test_kernel_inventory.py checks this list against the kernels of the built library, and that every test named here
exists).  A kernel added without an entry -- or without an fp64 test to name -- fails the CPU suite.

Names are the demangled kernel names without their parameter lists, as `nm -C` prints the library's host-side kernel handles.
KERNELS: name -> {"call": the entry point and arguments that launch it, "tests": test ids ("tests/<file>::<function>"; a
parametrized test is named by its function), "bounds": the tests of tests/test_buffers_gpu.py that run it on guarded buffers (stray
writes, stray reads, interior pointers, in place)}.  NOT_TRANSFORMS: name -> why the kernel has no fp64 comparison."""

PARITY = "tests/test_gpu_parity.py::"
PERCALL = "tests/test_percall_gpu.py::"
DIF = "tests/test_dif_gpu.py::"
FIR = "tests/test_fir_gpu.py::"
BOUNDS = "tests/test_buffers_gpu.py::"

KERNELS = {
    "FFT_GPU_R2C_C2R_external<FFT_256, FFT_forward>": {
        "call": "smfft_rc_external_benchmark / smfft_launch(family=2, path=0, N=512, inverse=0)",
        "tests": [PARITY + "test_r2c_c2r_vs_oracle_ragged"],
        "bounds": [BOUNDS + "test_rc_bounds", BOUNDS + "test_in_place_external"],
    },
    "FFT_GPU_R2C_C2R_external<FFT_256, FFT_inverse>": {
        "call": "smfft_rc_external_benchmark / smfft_launch(family=2, path=0, N=512, inverse=1)",
        "tests": [PARITY + "test_r2c_c2r_vs_oracle_ragged"],
        "bounds": [BOUNDS + "test_rc_bounds", BOUNDS + "test_in_place_external"],
    },
    "FFT_GPU_R2C_C2R_external<FFT_512, FFT_forward>": {
        "call": "smfft_rc_external_benchmark / smfft_launch(family=2, path=0, N=1024, inverse=0)",
        "tests": [PARITY + "test_r2c_c2r_vs_oracle_ragged"],
        "bounds": [BOUNDS + "test_rc_bounds", BOUNDS + "test_in_place_external", BOUNDS + "test_benchmark_forms"],
    },
    "FFT_GPU_R2C_C2R_external<FFT_512, FFT_inverse>": {
        "call": "smfft_rc_external_benchmark / smfft_launch(family=2, path=0, N=1024, inverse=1)",
        "tests": [PARITY + "test_r2c_c2r_vs_oracle_ragged"],
        "bounds": [BOUNDS + "test_rc_bounds", BOUNDS + "test_in_place_external", BOUNDS + "test_benchmark_forms"],
    },
    "FFT_GPU_R2C_C2R_external<FFT_1024, FFT_forward>": {
        "call": "smfft_rc_external_benchmark / smfft_launch(family=2, path=0, N=2048, inverse=0)",
        "tests": [PARITY + "test_r2c_c2r_vs_oracle_ragged"],
        "bounds": [BOUNDS + "test_rc_bounds"],
    },
    "FFT_GPU_R2C_C2R_external<FFT_1024, FFT_inverse>": {
        "call": "smfft_rc_external_benchmark / smfft_launch(family=2, path=0, N=2048, inverse=1)",
        "tests": [PARITY + "test_r2c_c2r_vs_oracle_ragged"],
        "bounds": [BOUNDS + "test_rc_bounds"],
    },
    "FFT_GPU_R2C_C2R_external<FFT_2048, FFT_forward>": {
        "call": "smfft_rc_external_benchmark / smfft_launch(family=2, path=0, N=4096, inverse=0)",
        "tests": [PARITY + "test_r2c_c2r_vs_oracle_ragged"],
        "bounds": [BOUNDS + "test_rc_bounds", BOUNDS + "test_in_place_external"],
    },
    "FFT_GPU_R2C_C2R_external<FFT_2048, FFT_inverse>": {
        "call": "smfft_rc_external_benchmark / smfft_launch(family=2, path=0, N=4096, inverse=1)",
        "tests": [PARITY + "test_r2c_c2r_vs_oracle_ragged"],
        "bounds": [BOUNDS + "test_rc_bounds", BOUNDS + "test_in_place_external"],
    },
    "FFT_GPU_R2C_C2R_multiple<FFT_256, FFT_forward>": {
        "call": "smfft_rc_multiple_benchmark / smfft_launch(family=2, path=1 or 2, N=512, inverse=0)",
        "tests": [PARITY + "test_r2c_multiple_k_applications"],
        "bounds": [BOUNDS + "test_rc_bounds"],
    },
    "FFT_GPU_R2C_C2R_multiple<FFT_256, FFT_inverse>": {
        "call": "smfft_launch(family=2, path=1 or 2, N=512, inverse=1)",
        "tests": [PARITY + "test_c2r_multiple_extension", PERCALL + "test_c2r_multiple_chains"],
        "bounds": [BOUNDS + "test_rc_bounds"],
    },
    "FFT_GPU_R2C_C2R_multiple<FFT_512, FFT_forward>": {
        "call": "smfft_rc_multiple_benchmark / smfft_launch(family=2, path=1 or 2, N=1024, inverse=0)",
        "tests": [PARITY + "test_r2c_multiple_k_applications"],
        "bounds": [BOUNDS + "test_rc_bounds", BOUNDS + "test_in_place_multiple_cut_chains", BOUNDS + "test_benchmark_forms"],
    },
    "FFT_GPU_R2C_C2R_multiple<FFT_512, FFT_inverse>": {
        "call": "smfft_launch(family=2, path=1 or 2, N=1024, inverse=1)",
        "tests": [PARITY + "test_c2r_multiple_extension", PERCALL + "test_c2r_multiple_chains"],
        "bounds": [BOUNDS + "test_rc_bounds"],
    },
    "FFT_GPU_R2C_C2R_multiple<FFT_1024, FFT_forward>": {
        "call": "smfft_rc_multiple_benchmark / smfft_launch(family=2, path=1 or 2, N=2048, inverse=0)",
        "tests": [PARITY + "test_r2c_multiple_k_applications"],
        "bounds": [BOUNDS + "test_rc_bounds"],
    },
    "FFT_GPU_R2C_C2R_multiple<FFT_1024, FFT_inverse>": {
        "call": "smfft_launch(family=2, path=1 or 2, N=2048, inverse=1)",
        "tests": [PARITY + "test_c2r_multiple_extension", PERCALL + "test_c2r_multiple_chains"],
        "bounds": [BOUNDS + "test_rc_bounds"],
    },
    "FFT_GPU_R2C_C2R_multiple<FFT_2048, FFT_forward>": {
        "call": "smfft_rc_multiple_benchmark / smfft_launch(family=2, path=1 or 2, N=4096, inverse=0)",
        "tests": [PARITY + "test_r2c_multiple_k_applications"],
        "bounds": [BOUNDS + "test_rc_bounds"],
    },
    "FFT_GPU_R2C_C2R_multiple<FFT_2048, FFT_inverse>": {
        "call": "smfft_launch(family=2, path=1 or 2, N=4096, inverse=1)",
        "tests": [PARITY + "test_c2r_multiple_extension", PERCALL + "test_c2r_multiple_chains"],
        "bounds": [BOUNDS + "test_rc_bounds", BOUNDS + "test_in_place_multiple_cut_chains"],
    },
    "FFT_GPU_external<FFT_32>": {
        "call": "smfft_st_external_benchmark / smfft_launch(family=1, path=0, N=32, inverse=1)",
        "tests": [PARITY + "test_stockham_external_golden"],
        "bounds": [BOUNDS + "test_stockham_bounds", BOUNDS + "test_in_place_external"],
    },
    "FFT_GPU_external<FFT_64>": {
        "call": "smfft_st_external_benchmark / smfft_launch(family=1, path=0, N=64, inverse=1)",
        "tests": [PARITY + "test_stockham_external_golden"],
        "bounds": [BOUNDS + "test_stockham_bounds"],
    },
    "FFT_GPU_external<FFT_128>": {
        "call": "smfft_st_external_benchmark / smfft_launch(family=1, path=0, N=128, inverse=1)",
        "tests": [PARITY + "test_stockham_external_golden"],
        "bounds": [BOUNDS + "test_stockham_bounds"],
    },
    "FFT_GPU_external<FFT_256>": {
        "call": "smfft_st_external_benchmark / smfft_launch(family=1, path=0, N=256, inverse=1)",
        "tests": [PARITY + "test_stockham_external_golden"],
        "bounds": [BOUNDS + "test_stockham_bounds", BOUNDS + "test_benchmark_forms"],
    },
    "FFT_GPU_external<FFT_512>": {
        "call": "smfft_st_external_benchmark / smfft_launch(family=1, path=0, N=512, inverse=1)",
        "tests": [PARITY + "test_stockham_external_golden"],
        "bounds": [BOUNDS + "test_stockham_bounds"],
    },
    "FFT_GPU_external<FFT_1024>": {
        "call": "smfft_st_external_benchmark / smfft_launch(family=1, path=0, N=1024, inverse=1)",
        "tests": [PARITY + "test_stockham_external_golden"],
        "bounds": [BOUNDS + "test_stockham_bounds", BOUNDS + "test_in_place_external"],
    },
    "FFT_GPU_external<FFT_2048>": {
        "call": "smfft_st_external_benchmark / smfft_launch(family=1, path=0, N=2048, inverse=1)",
        "tests": [PARITY + "test_stockham_external_golden"],
        "bounds": [BOUNDS + "test_stockham_bounds"],
    },
    "FFT_GPU_multiple<FFT_32>": {
        "call": "smfft_st_multiple_benchmark / smfft_launch(family=1, path=1 or 2, N=32, inverse=1)",
        "tests": [PARITY + "test_stockham_multiple_k_applications"],
        "bounds": [BOUNDS + "test_stockham_bounds"],
    },
    "FFT_GPU_multiple<FFT_64>": {
        "call": "smfft_st_multiple_benchmark / smfft_launch(family=1, path=1 or 2, N=64, inverse=1)",
        "tests": [PARITY + "test_stockham_multiple_k_applications"],
        "bounds": [BOUNDS + "test_stockham_bounds"],
    },
    "FFT_GPU_multiple<FFT_128>": {
        "call": "smfft_st_multiple_benchmark / smfft_launch(family=1, path=1 or 2, N=128, inverse=1)",
        "tests": [PARITY + "test_stockham_multiple_k_applications"],
        "bounds": [BOUNDS + "test_stockham_bounds"],
    },
    "FFT_GPU_multiple<FFT_256>": {
        "call": "smfft_st_multiple_benchmark / smfft_launch(family=1, path=1 or 2, N=256, inverse=1)",
        "tests": [PARITY + "test_stockham_multiple_k_applications"],
        "bounds": [BOUNDS + "test_stockham_bounds", BOUNDS + "test_benchmark_forms"],
    },
    "FFT_GPU_multiple<FFT_512>": {
        "call": "smfft_st_multiple_benchmark / smfft_launch(family=1, path=1 or 2, N=512, inverse=1)",
        "tests": [PARITY + "test_stockham_multiple_k_applications"],
        "bounds": [BOUNDS + "test_stockham_bounds"],
    },
    "FFT_GPU_multiple<FFT_1024>": {
        "call": "smfft_st_multiple_benchmark / smfft_launch(family=1, path=1 or 2, N=1024, inverse=1)",
        "tests": [PARITY + "test_stockham_multiple_k_applications"],
        "bounds": [BOUNDS + "test_stockham_bounds"],
    },
    "FFT_GPU_multiple<FFT_2048>": {
        "call": "smfft_st_multiple_benchmark / smfft_launch(family=1, path=1 or 2, N=2048, inverse=1)",
        "tests": [PARITY + "test_stockham_multiple_k_applications"],
        "bounds": [BOUNDS + "test_stockham_bounds", BOUNDS + "test_in_place_multiple_cut_chains"],
    },
    "FFT_GPU_multiple<FFT_4096>": {
        "call": "smfft_st_multiple_benchmark / smfft_launch(family=1, path=1 or 2, N=4096, inverse=1)",
        "tests": [PARITY + "test_stockham_multiple_k_applications"],
        "bounds": [BOUNDS + "test_stockham_bounds"],
    },
    "SMFFT_DIF_external<FFT_32_forward_noreorder>": {
        "call": "smfft_ct_dif_launch / smfft_ct_dif_external_benchmark(N=32, inverse=0)",
        "tests": [DIF + "test_library_dif_is_the_bit_reversed_dft"],
        "bounds": [BOUNDS + "test_dif_bounds", BOUNDS + "test_in_place_external"],
    },
    "SMFFT_DIF_external<FFT_32_inverse_noreorder>": {
        "call": "smfft_ct_dif_launch / smfft_ct_dif_external_benchmark(N=32, inverse=1)",
        "tests": [DIF + "test_library_dif_is_the_bit_reversed_dft"],
        "bounds": [BOUNDS + "test_dif_bounds", BOUNDS + "test_in_place_external"],
    },
    "SMFFT_DIF_external<FFT_64_forward_noreorder>": {
        "call": "smfft_ct_dif_launch / smfft_ct_dif_external_benchmark(N=64, inverse=0)",
        "tests": [DIF + "test_library_dif_is_the_bit_reversed_dft"],
        "bounds": [BOUNDS + "test_dif_bounds"],
    },
    "SMFFT_DIF_external<FFT_64_inverse_noreorder>": {
        "call": "smfft_ct_dif_launch / smfft_ct_dif_external_benchmark(N=64, inverse=1)",
        "tests": [DIF + "test_library_dif_is_the_bit_reversed_dft"],
        "bounds": [BOUNDS + "test_dif_bounds"],
    },
    "SMFFT_DIF_external<FFT_128_forward_noreorder>": {
        "call": "smfft_ct_dif_launch / smfft_ct_dif_external_benchmark(N=128, inverse=0)",
        "tests": [DIF + "test_library_dif_is_the_bit_reversed_dft"],
        "bounds": [BOUNDS + "test_dif_bounds"],
    },
    "SMFFT_DIF_external<FFT_128_inverse_noreorder>": {
        "call": "smfft_ct_dif_launch / smfft_ct_dif_external_benchmark(N=128, inverse=1)",
        "tests": [DIF + "test_library_dif_is_the_bit_reversed_dft"],
        "bounds": [BOUNDS + "test_dif_bounds"],
    },
    "SMFFT_DIF_external<FFT_256_forward_noreorder>": {
        "call": "smfft_ct_dif_launch / smfft_ct_dif_external_benchmark(N=256, inverse=0)",
        "tests": [DIF + "test_library_dif_is_the_bit_reversed_dft"],
        "bounds": [BOUNDS + "test_dif_bounds", BOUNDS + "test_benchmark_forms"],
    },
    "SMFFT_DIF_external<FFT_256_inverse_noreorder>": {
        "call": "smfft_ct_dif_launch / smfft_ct_dif_external_benchmark(N=256, inverse=1)",
        "tests": [DIF + "test_library_dif_is_the_bit_reversed_dft"],
        "bounds": [BOUNDS + "test_dif_bounds"],
    },
    "SMFFT_DIF_external<FFT_512_forward_noreorder>": {
        "call": "smfft_ct_dif_launch / smfft_ct_dif_external_benchmark(N=512, inverse=0)",
        "tests": [DIF + "test_library_dif_is_the_bit_reversed_dft"],
        "bounds": [BOUNDS + "test_dif_bounds"],
    },
    "SMFFT_DIF_external<FFT_512_inverse_noreorder>": {
        "call": "smfft_ct_dif_launch / smfft_ct_dif_external_benchmark(N=512, inverse=1)",
        "tests": [DIF + "test_library_dif_is_the_bit_reversed_dft"],
        "bounds": [BOUNDS + "test_dif_bounds"],
    },
    "SMFFT_DIF_external<FFT_1024_forward_noreorder>": {
        "call": "smfft_ct_dif_launch / smfft_ct_dif_external_benchmark(N=1024, inverse=0)",
        "tests": [DIF + "test_library_dif_is_the_bit_reversed_dft"],
        "bounds": [BOUNDS + "test_dif_bounds", BOUNDS + "test_in_place_external"],
    },
    "SMFFT_DIF_external<FFT_1024_inverse_noreorder>": {
        "call": "smfft_ct_dif_launch / smfft_ct_dif_external_benchmark(N=1024, inverse=1)",
        "tests": [DIF + "test_library_dif_is_the_bit_reversed_dft"],
        "bounds": [BOUNDS + "test_dif_bounds", BOUNDS + "test_in_place_external"],
    },
    "SMFFT_DIF_external<FFT_2048_forward_noreorder>": {
        "call": "smfft_ct_dif_launch / smfft_ct_dif_external_benchmark(N=2048, inverse=0)",
        "tests": [DIF + "test_library_dif_is_the_bit_reversed_dft"],
        "bounds": [BOUNDS + "test_dif_bounds"],
    },
    "SMFFT_DIF_external<FFT_2048_inverse_noreorder>": {
        "call": "smfft_ct_dif_launch / smfft_ct_dif_external_benchmark(N=2048, inverse=1)",
        "tests": [DIF + "test_library_dif_is_the_bit_reversed_dft"],
        "bounds": [BOUNDS + "test_dif_bounds"],
    },
    "SMFFT_DIF_external<FFT_4096_forward_noreorder>": {
        "call": "smfft_ct_dif_launch / smfft_ct_dif_external_benchmark(N=4096, inverse=0)",
        "tests": [DIF + "test_library_dif_is_the_bit_reversed_dft"],
        "bounds": [BOUNDS + "test_dif_bounds", BOUNDS + "test_in_place_external"],
    },
    "SMFFT_DIF_external<FFT_4096_inverse_noreorder>": {
        "call": "smfft_ct_dif_launch / smfft_ct_dif_external_benchmark(N=4096, inverse=1)",
        "tests": [DIF + "test_library_dif_is_the_bit_reversed_dft"],
        "bounds": [BOUNDS + "test_dif_bounds", BOUNDS + "test_in_place_external"],
    },
    "SMFFT_DIT_external<FFT_32_forward>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=32, inverse=0, reorder=1)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds", BOUNDS + "test_stockham_bounds", BOUNDS + "test_in_place_external"],
    },
    "SMFFT_DIT_external<FFT_32_forward_noreorder>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=32, inverse=0, reorder=0)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds", BOUNDS + "test_in_place_external"],
    },
    "SMFFT_DIT_external<FFT_32_inverse>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=32, inverse=1, reorder=1)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds", BOUNDS + "test_in_place_external"],
    },
    "SMFFT_DIT_external<FFT_32_inverse_noreorder>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=32, inverse=1, reorder=0)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds", BOUNDS + "test_in_place_external"],
    },
    "SMFFT_DIT_external<FFT_64_forward>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=64, inverse=0, reorder=1)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds", BOUNDS + "test_stockham_bounds"],
    },
    "SMFFT_DIT_external<FFT_64_forward_noreorder>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=64, inverse=0, reorder=0)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds"],
    },
    "SMFFT_DIT_external<FFT_64_inverse>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=64, inverse=1, reorder=1)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds"],
    },
    "SMFFT_DIT_external<FFT_64_inverse_noreorder>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=64, inverse=1, reorder=0)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds"],
    },
    "SMFFT_DIT_external<FFT_128_forward>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=128, inverse=0, reorder=1)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds", BOUNDS + "test_stockham_bounds"],
    },
    "SMFFT_DIT_external<FFT_128_forward_noreorder>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=128, inverse=0, reorder=0)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds"],
    },
    "SMFFT_DIT_external<FFT_128_inverse>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=128, inverse=1, reorder=1)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds"],
    },
    "SMFFT_DIT_external<FFT_128_inverse_noreorder>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=128, inverse=1, reorder=0)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds"],
    },
    "SMFFT_DIT_external<FFT_256_forward>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=256, inverse=0, reorder=1)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds", BOUNDS + "test_stockham_bounds", BOUNDS + "test_benchmark_forms"],
    },
    "SMFFT_DIT_external<FFT_256_forward_noreorder>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=256, inverse=0, reorder=0)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds"],
    },
    "SMFFT_DIT_external<FFT_256_inverse>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=256, inverse=1, reorder=1)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds"],
    },
    "SMFFT_DIT_external<FFT_256_inverse_noreorder>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=256, inverse=1, reorder=0)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds"],
    },
    "SMFFT_DIT_external<FFT_512_forward>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=512, inverse=0, reorder=1)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds", BOUNDS + "test_stockham_bounds"],
    },
    "SMFFT_DIT_external<FFT_512_forward_noreorder>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=512, inverse=0, reorder=0)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds"],
    },
    "SMFFT_DIT_external<FFT_512_inverse>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=512, inverse=1, reorder=1)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds"],
    },
    "SMFFT_DIT_external<FFT_512_inverse_noreorder>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=512, inverse=1, reorder=0)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds"],
    },
    "SMFFT_DIT_external<FFT_1024_forward>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=1024, inverse=0, reorder=1)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds", BOUNDS + "test_stockham_bounds", BOUNDS + "test_in_place_external"],
    },
    "SMFFT_DIT_external<FFT_1024_forward_noreorder>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=1024, inverse=0, reorder=0)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds", BOUNDS + "test_in_place_external"],
    },
    "SMFFT_DIT_external<FFT_1024_inverse>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=1024, inverse=1, reorder=1)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds", BOUNDS + "test_in_place_external"],
    },
    "SMFFT_DIT_external<FFT_1024_inverse_noreorder>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=1024, inverse=1, reorder=0)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds", BOUNDS + "test_in_place_external"],
    },
    "SMFFT_DIT_external<FFT_2048_forward>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=2048, inverse=0, reorder=1)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds", BOUNDS + "test_stockham_bounds"],
    },
    "SMFFT_DIT_external<FFT_2048_forward_noreorder>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=2048, inverse=0, reorder=0)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds"],
    },
    "SMFFT_DIT_external<FFT_2048_inverse>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=2048, inverse=1, reorder=1)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds"],
    },
    "SMFFT_DIT_external<FFT_2048_inverse_noreorder>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=2048, inverse=1, reorder=0)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds"],
    },
    "SMFFT_DIT_external<FFT_4096_forward_noreorder>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=4096, inverse=0, reorder=0)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds", BOUNDS + "test_in_place_external"],
    },
    "SMFFT_DIT_external<FFT_4096_inverse_noreorder>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=4096, inverse=1, reorder=0)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds", BOUNDS + "test_in_place_external"],
    },
    "SMFFT_DIT_external_occ3<FFT_4096_forward>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=4096, inverse=0, reorder=1)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds", BOUNDS + "test_stockham_bounds", BOUNDS + "test_in_place_external"],
    },
    "SMFFT_DIT_external_occ3<FFT_4096_inverse>": {
        "call": "smfft_ct_external_benchmark / smfft_launch(family=0, path=0, N=4096, inverse=1, reorder=1); smfft_st_external_benchmark(N=4096)",
        "tests": [PARITY + "test_ct_external_vs_oracle_ragged", PARITY + "test_ct_external_golden", PARITY + "test_stockham_external_golden"],
        "bounds": [BOUNDS + "test_ct_external_bounds", BOUNDS + "test_stockham_bounds", BOUNDS + "test_in_place_external"],
    },
    "SMFFT_DIT_multiple<FFT_32_forward>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=32, inverse=0, reorder=1); smfft_launch(family=1, path=1, inverse=0)",
        "tests": [PARITY + "test_ct_multiple_k_applications", PERCALL + "test_stockham_forward_multiple_launch"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds", BOUNDS + "test_stockham_bounds", BOUNDS + "test_in_place_multiple_cut_chains"],
    },
    "SMFFT_DIT_multiple<FFT_32_forward_noreorder>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=32, inverse=0, reorder=0)",
        "tests": [PARITY + "test_ct_multiple_k_applications"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple<FFT_32_inverse>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=32, inverse=1, reorder=1)",
        "tests": [PARITY + "test_ct_multiple_k_applications"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple<FFT_32_inverse_noreorder>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=32, inverse=1, reorder=0)",
        "tests": [PARITY + "test_ct_multiple_k_applications"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple<FFT_64_forward>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=64, inverse=0, reorder=1); smfft_launch(family=1, path=1, inverse=0)",
        "tests": [PARITY + "test_ct_multiple_k_applications", PERCALL + "test_stockham_forward_multiple_launch"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds", BOUNDS + "test_stockham_bounds"],
    },
    "SMFFT_DIT_multiple<FFT_64_forward_noreorder>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=64, inverse=0, reorder=0)",
        "tests": [PARITY + "test_ct_multiple_k_applications"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple<FFT_64_inverse>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=64, inverse=1, reorder=1)",
        "tests": [PARITY + "test_ct_multiple_k_applications"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple<FFT_64_inverse_noreorder>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=64, inverse=1, reorder=0)",
        "tests": [PARITY + "test_ct_multiple_k_applications"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds", BOUNDS + "test_in_place_multiple_cut_chains"],
    },
    "SMFFT_DIT_multiple<FFT_128_forward>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=128, inverse=0, reorder=1); smfft_launch(family=1, path=1, inverse=0)",
        "tests": [PARITY + "test_ct_multiple_k_applications", PERCALL + "test_stockham_forward_multiple_launch"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds", BOUNDS + "test_stockham_bounds"],
    },
    "SMFFT_DIT_multiple<FFT_128_forward_noreorder>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=128, inverse=0, reorder=0); the same kernel on path=2",
        "tests": [PARITY + "test_ct_multiple_k_applications", PERCALL + "test_percall_path_against_fp64_and_path1"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple<FFT_128_inverse>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=128, inverse=1, reorder=1)",
        "tests": [PARITY + "test_ct_multiple_k_applications"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple<FFT_128_inverse_noreorder>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=128, inverse=1, reorder=0); the same kernel on path=2",
        "tests": [PARITY + "test_ct_multiple_k_applications", PERCALL + "test_percall_path_against_fp64_and_path1"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple<FFT_256_forward>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=256, inverse=0, reorder=1); smfft_launch(family=1, path=1, inverse=0)",
        "tests": [PARITY + "test_ct_multiple_k_applications", PERCALL + "test_stockham_forward_multiple_launch"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds", BOUNDS + "test_stockham_bounds", BOUNDS + "test_in_place_late_owner"],
    },
    "SMFFT_DIT_multiple<FFT_256_forward_noreorder>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=256, inverse=0, reorder=0); the same kernel on path=2",
        "tests": [PARITY + "test_ct_multiple_k_applications", PERCALL + "test_percall_path_against_fp64_and_path1"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds", BOUNDS + "test_in_place_multiple_cut_chains"],
    },
    "SMFFT_DIT_multiple<FFT_256_inverse>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=256, inverse=1, reorder=1)",
        "tests": [PARITY + "test_ct_multiple_k_applications"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds", BOUNDS + "test_benchmark_forms"],
    },
    "SMFFT_DIT_multiple<FFT_256_inverse_noreorder>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=256, inverse=1, reorder=0); the same kernel on path=2",
        "tests": [PARITY + "test_ct_multiple_k_applications", PERCALL + "test_percall_path_against_fp64_and_path1"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple<FFT_512_forward>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=512, inverse=0, reorder=1); smfft_launch(family=1, path=1, inverse=0)",
        "tests": [PARITY + "test_ct_multiple_k_applications", PERCALL + "test_stockham_forward_multiple_launch"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds", BOUNDS + "test_stockham_bounds"],
    },
    "SMFFT_DIT_multiple<FFT_512_forward_noreorder>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=512, inverse=0, reorder=0); the same kernel on path=2",
        "tests": [PARITY + "test_ct_multiple_k_applications", PERCALL + "test_percall_path_against_fp64_and_path1"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple<FFT_512_inverse>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=512, inverse=1, reorder=1)",
        "tests": [PARITY + "test_ct_multiple_k_applications"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple<FFT_512_inverse_noreorder>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=512, inverse=1, reorder=0); the same kernel on path=2",
        "tests": [PARITY + "test_ct_multiple_k_applications", PERCALL + "test_percall_path_against_fp64_and_path1"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple<FFT_1024_forward>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=1024, inverse=0, reorder=1); smfft_launch(family=1, path=1, inverse=0)",
        "tests": [PARITY + "test_ct_multiple_k_applications", PERCALL + "test_stockham_forward_multiple_launch"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds", BOUNDS + "test_stockham_bounds"],
    },
    "SMFFT_DIT_multiple<FFT_1024_forward_noreorder>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=1024, inverse=0, reorder=0); the same kernel on path=2",
        "tests": [PARITY + "test_ct_multiple_k_applications", PERCALL + "test_percall_path_against_fp64_and_path1"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple<FFT_1024_inverse>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=1024, inverse=1, reorder=1)",
        "tests": [PARITY + "test_ct_multiple_k_applications"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds", BOUNDS + "test_in_place_multiple_cut_chains"],
    },
    "SMFFT_DIT_multiple<FFT_1024_inverse_noreorder>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=1024, inverse=1, reorder=0); the same kernel on path=2",
        "tests": [PARITY + "test_ct_multiple_k_applications", PERCALL + "test_percall_path_against_fp64_and_path1"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple<FFT_2048_forward>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=2048, inverse=0, reorder=1); smfft_launch(family=1, path=1, inverse=0)",
        "tests": [PARITY + "test_ct_multiple_k_applications", PERCALL + "test_stockham_forward_multiple_launch"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds", BOUNDS + "test_stockham_bounds"],
    },
    "SMFFT_DIT_multiple<FFT_2048_forward_noreorder>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=2048, inverse=0, reorder=0); the same kernel on path=2",
        "tests": [PARITY + "test_ct_multiple_k_applications", PERCALL + "test_percall_path_against_fp64_and_path1"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple<FFT_2048_inverse>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=2048, inverse=1, reorder=1)",
        "tests": [PARITY + "test_ct_multiple_k_applications"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple<FFT_2048_inverse_noreorder>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=2048, inverse=1, reorder=0); the same kernel on path=2",
        "tests": [PARITY + "test_ct_multiple_k_applications", PERCALL + "test_percall_path_against_fp64_and_path1"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple<FFT_4096_forward>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=4096, inverse=0, reorder=1); smfft_launch(family=1, path=1, inverse=0)",
        "tests": [PARITY + "test_ct_multiple_k_applications", PERCALL + "test_stockham_forward_multiple_launch"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds", BOUNDS + "test_stockham_bounds", BOUNDS + "test_in_place_multiple_cut_chains"],
    },
    "SMFFT_DIT_multiple<FFT_4096_forward_noreorder>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=4096, inverse=0, reorder=0); the same kernel on path=2",
        "tests": [PARITY + "test_ct_multiple_k_applications", PERCALL + "test_percall_path_against_fp64_and_path1"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple<FFT_4096_inverse>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=4096, inverse=1, reorder=1)",
        "tests": [PARITY + "test_ct_multiple_k_applications"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple<FFT_4096_inverse_noreorder>": {
        "call": "smfft_ct_multiple_benchmark / smfft_launch(family=0, path=1, N=4096, inverse=1, reorder=0); the same kernel on path=2",
        "tests": [PARITY + "test_ct_multiple_k_applications", PERCALL + "test_percall_path_against_fp64_and_path1"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple_unfused<FFT_32_forward>": {
        "call": "smfft_ct_multiple_percall_benchmark / smfft_launch(family=0, path=2, N=32, inverse=0, reorder=1); smfft_ct_multiple_unfused_benchmark; smfft_launch(family=1, path=2, inverse=0)",
        "tests": [PERCALL + "test_percall_path_against_fp64_and_path1", PERCALL + "test_percall_balanced_schedule_is_bit_identical", PERCALL + "test_percall_long_chains_against_the_oracle", PERCALL + "test_stockham_forward_multiple_launch"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds", BOUNDS + "test_stockham_bounds", BOUNDS + "test_in_place_multiple_cut_chains"],
    },
    "SMFFT_DIT_multiple_unfused<FFT_32_forward_noreorder>": {
        "call": "smfft_ct_multiple_percall_benchmark / smfft_launch(family=0, path=2, N=32, inverse=0, reorder=0)",
        "tests": [PERCALL + "test_percall_path_against_fp64_and_path1", PERCALL + "test_percall_balanced_schedule_is_bit_identical", PERCALL + "test_percall_long_chains_against_the_oracle"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple_unfused<FFT_32_inverse>": {
        "call": "smfft_ct_multiple_percall_benchmark / smfft_launch(family=0, path=2, N=32, inverse=1, reorder=1); smfft_ct_multiple_unfused_benchmark",
        "tests": [PERCALL + "test_percall_path_against_fp64_and_path1", PERCALL + "test_percall_balanced_schedule_is_bit_identical", PERCALL + "test_percall_long_chains_against_the_oracle"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple_unfused<FFT_32_inverse_noreorder>": {
        "call": "smfft_ct_multiple_percall_benchmark / smfft_launch(family=0, path=2, N=32, inverse=1, reorder=0)",
        "tests": [PERCALL + "test_percall_path_against_fp64_and_path1", PERCALL + "test_percall_balanced_schedule_is_bit_identical", PERCALL + "test_percall_long_chains_against_the_oracle"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple_unfused<FFT_64_forward>": {
        "call": "smfft_ct_multiple_percall_benchmark / smfft_launch(family=0, path=2, N=64, inverse=0, reorder=1); smfft_ct_multiple_unfused_benchmark; smfft_launch(family=1, path=2, inverse=0)",
        "tests": [PERCALL + "test_percall_path_against_fp64_and_path1", PERCALL + "test_percall_balanced_schedule_is_bit_identical", PERCALL + "test_stockham_forward_multiple_launch"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds", BOUNDS + "test_stockham_bounds"],
    },
    "SMFFT_DIT_multiple_unfused<FFT_64_forward_noreorder>": {
        "call": "smfft_ct_multiple_percall_benchmark / smfft_launch(family=0, path=2, N=64, inverse=0, reorder=0)",
        "tests": [PERCALL + "test_percall_path_against_fp64_and_path1", PERCALL + "test_percall_balanced_schedule_is_bit_identical", PERCALL + "test_percall_long_chains_against_the_oracle"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple_unfused<FFT_64_inverse>": {
        "call": "smfft_ct_multiple_percall_benchmark / smfft_launch(family=0, path=2, N=64, inverse=1, reorder=1); smfft_ct_multiple_unfused_benchmark",
        "tests": [PERCALL + "test_percall_path_against_fp64_and_path1", PERCALL + "test_percall_balanced_schedule_is_bit_identical"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple_unfused<FFT_64_inverse_noreorder>": {
        "call": "smfft_ct_multiple_percall_benchmark / smfft_launch(family=0, path=2, N=64, inverse=1, reorder=0)",
        "tests": [PERCALL + "test_percall_path_against_fp64_and_path1", PERCALL + "test_percall_balanced_schedule_is_bit_identical", PERCALL + "test_percall_long_chains_against_the_oracle"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds", BOUNDS + "test_in_place_multiple_cut_chains"],
    },
    "SMFFT_DIT_multiple_unfused<FFT_128_forward>": {
        "call": "smfft_ct_multiple_percall_benchmark / smfft_launch(family=0, path=2, N=128, inverse=0, reorder=1); smfft_ct_multiple_unfused_benchmark; smfft_launch(family=1, path=2, inverse=0)",
        "tests": [PERCALL + "test_percall_path_against_fp64_and_path1", PERCALL + "test_percall_balanced_schedule_is_bit_identical", PERCALL + "test_stockham_forward_multiple_launch"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds", BOUNDS + "test_stockham_bounds"],
    },
    "SMFFT_DIT_multiple_unfused<FFT_128_inverse>": {
        "call": "smfft_ct_multiple_percall_benchmark / smfft_launch(family=0, path=2, N=128, inverse=1, reorder=1); smfft_ct_multiple_unfused_benchmark",
        "tests": [PERCALL + "test_percall_path_against_fp64_and_path1", PERCALL + "test_percall_balanced_schedule_is_bit_identical"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple_unfused<FFT_256_forward>": {
        "call": "smfft_ct_multiple_percall_benchmark / smfft_launch(family=0, path=2, N=256, inverse=0, reorder=1); smfft_ct_multiple_unfused_benchmark; smfft_launch(family=1, path=2, inverse=0)",
        "tests": [PERCALL + "test_percall_path_against_fp64_and_path1", PERCALL + "test_percall_balanced_schedule_is_bit_identical", PERCALL + "test_stockham_forward_multiple_launch"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds", BOUNDS + "test_stockham_bounds", BOUNDS + "test_benchmark_forms"],
    },
    "SMFFT_DIT_multiple_unfused<FFT_256_inverse>": {
        "call": "smfft_ct_multiple_percall_benchmark / smfft_launch(family=0, path=2, N=256, inverse=1, reorder=1); smfft_ct_multiple_unfused_benchmark",
        "tests": [PERCALL + "test_percall_path_against_fp64_and_path1", PERCALL + "test_percall_balanced_schedule_is_bit_identical"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple_unfused<FFT_512_forward>": {
        "call": "smfft_ct_multiple_percall_benchmark / smfft_launch(family=0, path=2, N=512, inverse=0, reorder=1); smfft_ct_multiple_unfused_benchmark; smfft_launch(family=1, path=2, inverse=0)",
        "tests": [PERCALL + "test_percall_path_against_fp64_and_path1", PERCALL + "test_percall_balanced_schedule_is_bit_identical", PERCALL + "test_stockham_forward_multiple_launch"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds", BOUNDS + "test_stockham_bounds"],
    },
    "SMFFT_DIT_multiple_unfused<FFT_512_inverse>": {
        "call": "smfft_ct_multiple_percall_benchmark / smfft_launch(family=0, path=2, N=512, inverse=1, reorder=1); smfft_ct_multiple_unfused_benchmark",
        "tests": [PERCALL + "test_percall_path_against_fp64_and_path1", PERCALL + "test_percall_balanced_schedule_is_bit_identical"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple_unfused<FFT_1024_forward>": {
        "call": "smfft_ct_multiple_percall_benchmark / smfft_launch(family=0, path=2, N=1024, inverse=0, reorder=1); smfft_ct_multiple_unfused_benchmark; smfft_launch(family=1, path=2, inverse=0)",
        "tests": [PERCALL + "test_percall_path_against_fp64_and_path1", PERCALL + "test_percall_balanced_schedule_is_bit_identical", PERCALL + "test_stockham_forward_multiple_launch"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds", BOUNDS + "test_stockham_bounds"],
    },
    "SMFFT_DIT_multiple_unfused<FFT_1024_inverse>": {
        "call": "smfft_ct_multiple_percall_benchmark / smfft_launch(family=0, path=2, N=1024, inverse=1, reorder=1); smfft_ct_multiple_unfused_benchmark",
        "tests": [PERCALL + "test_percall_path_against_fp64_and_path1", PERCALL + "test_percall_balanced_schedule_is_bit_identical"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds", BOUNDS + "test_in_place_multiple_cut_chains"],
    },
    "SMFFT_DIT_multiple_unfused<FFT_2048_forward>": {
        "call": "smfft_ct_multiple_percall_benchmark / smfft_launch(family=0, path=2, N=2048, inverse=0, reorder=1); smfft_ct_multiple_unfused_benchmark; smfft_launch(family=1, path=2, inverse=0)",
        "tests": [PERCALL + "test_percall_path_against_fp64_and_path1", PERCALL + "test_percall_balanced_schedule_is_bit_identical", PERCALL + "test_stockham_forward_multiple_launch"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds", BOUNDS + "test_stockham_bounds"],
    },
    "SMFFT_DIT_multiple_unfused<FFT_2048_inverse>": {
        "call": "smfft_ct_multiple_percall_benchmark / smfft_launch(family=0, path=2, N=2048, inverse=1, reorder=1); smfft_ct_multiple_unfused_benchmark",
        "tests": [PERCALL + "test_percall_path_against_fp64_and_path1", PERCALL + "test_percall_balanced_schedule_is_bit_identical"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "SMFFT_DIT_multiple_unfused<FFT_4096_forward>": {
        "call": "smfft_ct_multiple_percall_benchmark / smfft_launch(family=0, path=2, N=4096, inverse=0, reorder=1); smfft_ct_multiple_unfused_benchmark; smfft_launch(family=1, path=2, inverse=0)",
        "tests": [PERCALL + "test_percall_path_against_fp64_and_path1", PERCALL + "test_percall_balanced_schedule_is_bit_identical", PERCALL + "test_stockham_forward_multiple_launch"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds", BOUNDS + "test_stockham_bounds", BOUNDS + "test_in_place_multiple_cut_chains"],
    },
    "SMFFT_DIT_multiple_unfused<FFT_4096_inverse>": {
        "call": "smfft_ct_multiple_percall_benchmark / smfft_launch(family=0, path=2, N=4096, inverse=1, reorder=1); smfft_ct_multiple_unfused_benchmark",
        "tests": [PERCALL + "test_percall_path_against_fp64_and_path1", PERCALL + "test_percall_balanced_schedule_is_bit_identical"],
        "bounds": [BOUNDS + "test_ct_multiple_bounds"],
    },
    "smfft::(anonymous namespace)::fir_overlap_save_kernel<256>": {
        "call": "smfft_fir_launch(FFT_size=256, correlate=0 or 1)",
        "tests": [FIR + "test_filter_bank_matches_numpy", FIR + "test_grid_stride_loop_with_wrapped_prefetch", FIR + "test_uneven_filter_groups"],
        "bounds": [BOUNDS + "test_fir_bounds"],
    },
    "smfft::(anonymous namespace)::fir_overlap_save_kernel<512>": {
        "call": "smfft_fir_launch(FFT_size=512, correlate=0 or 1)",
        "tests": [FIR + "test_filter_bank_matches_numpy", FIR + "test_grid_stride_loop_with_wrapped_prefetch"],
        "bounds": [BOUNDS + "test_fir_bounds"],
    },
    "smfft::(anonymous namespace)::fir_overlap_save_kernel<1024>": {
        "call": "smfft_fir_launch(FFT_size=1024, correlate=0 or 1)",
        "tests": [FIR + "test_filter_bank_matches_numpy", FIR + "test_grid_stride_loop_with_wrapped_prefetch", FIR + "test_grid_stride_loop_at_a_realistic_shape"],
        "bounds": [BOUNDS + "test_fir_bounds", BOUNDS + "test_benchmark_forms"],
    },
    "smfft::(anonymous namespace)::fir_overlap_save_kernel<2048>": {
        "call": "smfft_fir_launch(FFT_size=2048, correlate=0 or 1)",
        "tests": [FIR + "test_filter_bank_matches_numpy", FIR + "test_grid_stride_loop_with_wrapped_prefetch"],
        "bounds": [BOUNDS + "test_fir_bounds"],
    },
    "smfft::(anonymous namespace)::fir_overlap_save_kernel<4096>": {
        "call": "smfft_fir_launch(FFT_size=4096, correlate=0 or 1)",
        "tests": [FIR + "test_filter_bank_matches_numpy", FIR + "test_grid_stride_loop_with_wrapped_prefetch", FIR + "test_uneven_filter_groups"],
        "bounds": [BOUNDS + "test_fir_bounds"],
    },
    "smfft::(anonymous namespace)::fir_prepare_kernel<256>": {
        "call": "smfft_fir_prepare(FFT_size=256, correlate=0 or 1)",
        "tests": [FIR + "test_prepared_spectra"],
        "bounds": [BOUNDS + "test_fir_bounds"],
    },
    "smfft::(anonymous namespace)::fir_prepare_kernel<512>": {
        "call": "smfft_fir_prepare(FFT_size=512, correlate=0 or 1)",
        "tests": [FIR + "test_prepared_spectra"],
        "bounds": [BOUNDS + "test_fir_bounds"],
    },
    "smfft::(anonymous namespace)::fir_prepare_kernel<1024>": {
        "call": "smfft_fir_prepare(FFT_size=1024, correlate=0 or 1)",
        "tests": [FIR + "test_prepared_spectra"],
        "bounds": [BOUNDS + "test_fir_bounds", BOUNDS + "test_benchmark_forms"],
    },
    "smfft::(anonymous namespace)::fir_prepare_kernel<2048>": {
        "call": "smfft_fir_prepare(FFT_size=2048, correlate=0 or 1)",
        "tests": [FIR + "test_prepared_spectra"],
        "bounds": [BOUNDS + "test_fir_bounds"],
    },
    "smfft::(anonymous namespace)::fir_prepare_kernel<4096>": {
        "call": "smfft_fir_prepare(FFT_size=4096, correlate=0 or 1)",
        "tests": [FIR + "test_prepared_spectra"],
        "bounds": [BOUNDS + "test_fir_bounds"],
    },
}

NOT_TRANSFORMS = {
    "SMFFT_stream_copy<0>": "no transform: a copy with the external kernels' access shape (smfft_copy_launch, bench.py's copy ceiling, the pair allocator's placement probes)",
    "SMFFT_stream_read<0>": "no transform: the read half of that copy, a probe of the pair allocator's placement search (smfft_pairs.hip)",
    "SMFFT_stream_write<0>": "no transform: the write half of that copy, a probe of the pair allocator's placement search (smfft_pairs.hip)",
}

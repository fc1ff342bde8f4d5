// dif_convolution.hip -- user kernels on the reference's contract (blockDim.x = fft_length / 4, README.md:10-18) that call the
// decimation-in-frequency transform of include/smfft/smfft_dif.hpp: natural order in, bit-reversed spectrum out.  The bit-reversed
// order is what the reference's fft_reorder = 0 exists for (README.md:12-14: "might not be always required for example for
// convolutions"): a filter applied in the same order as the transformed data, and the no-reorder inverse transform takes that order
// back to natural order -- neither transform reorders anything.  tests/test_dif_gpu.py runs everything here against numpy.
//
// Build: hipcc -O3 --offload-arch=gfx950 -std=c++17 -fPIC -shared -I include examples/dif_convolution.hip
#include <hip/hip_runtime.h>
#include <smfft_device.hpp>

// fill / do_SMFFT_CT_DIF / drain, exactly as user_fft_kernel of reference_shape_kernel.hip does around do_SMFFT_CT_DIT
template <class const_params>
__global__ void user_dif_kernel(const float2* d_input, float2* d_output) {
    __shared__ float2 s_data[const_params::fft_sm_required];
    const size_t offset = (size_t)blockIdx.x * const_params::fft_length;
    for (int k = 0; k < 4; k++) s_data[threadIdx.x + k * const_params::fft_length_quarter] = d_input[offset + threadIdx.x + k * const_params::fft_length_quarter];
    __syncthreads();
    do_SMFFT_CT_DIF<const_params>(s_data);
    __syncthreads();
    for (int k = 0; k < 4; k++) d_output[offset + threadIdx.x + k * const_params::fft_length_quarter] = s_data[threadIdx.x + k * const_params::fft_length_quarter];
}
// the register form (N >= 256): the coalesced load is the first pass's input, the thread ends with positions 4 threadIdx.x + k
template <class const_params>
__global__ void __launch_bounds__(const_params::fft_length_quarter) user_dif_kernel_registers(const float2* d_input, float2* d_output) {
    __shared__ float2 s_scratch[const_params::fft_sm_required];
    constexpr int Q = const_params::fft_length_quarter;
    const size_t offset = (size_t)blockIdx.x * const_params::fft_length;
    float2 x[4];
    for (int k = 0; k < 4; k++) x[k] = d_input[offset + threadIdx.x + k * Q];
    do_SMFFT_CT_DIF_registers<const_params>(x, s_scratch);
    for (int k = 0; k < 4; k++) d_output[offset + 4 * threadIdx.x + k] = x[k];
}

template <class P>
static int launch_dif(const float2* in, float2* out, int nFFTs, int which, hipStream_t st) {
    // the reference's launch arithmetic (CT:586-595): fft_length / N transforms per block of fft_length / 4 threads
    const dim3 grid(nFFTs / (P::fft_length / P::fft_size)), block(P::fft_length / 4);
    if (grid.x == 0) return 0;
    if constexpr (P::fft_size >= 256) {
        if (which == 1) {
            user_dif_kernel_registers<P><<<grid, block, 0, st>>>(in, out);
            return (int)hipGetLastError();
        }
    }
    user_dif_kernel<P><<<grid, block, 0, st>>>(in, out);
    return (int)hipGetLastError();
}
#define DIF_CASE_SMALL(N)                                                                                                      \
    case N:                                                                                                                    \
        if (which == 2) return inverse ? launch_dif<FFT_##N##_inverse_noreorder_wave64>(in, out, nFFTs, which, st)            \
                                       : launch_dif<FFT_##N##_forward_noreorder_wave64>(in, out, nFFTs, which, st);           \
        if (which != 0) return -1;                                                                                             \
        return inverse ? launch_dif<FFT_##N##_inverse_noreorder>(in, out, nFFTs, which, st) : launch_dif<FFT_##N##_forward_noreorder>(in, out, nFFTs, which, st);
#define DIF_CASE(N)                                                                                                            \
    case N:                                                                                                                    \
        if (which > 1) return -1;                                                                                              \
        return inverse ? launch_dif<FFT_##N##_inverse_noreorder>(in, out, nFFTs, which, st) : launch_dif<FFT_##N##_forward_noreorder>(in, out, nFFTs, which, st);

// which = 0: fill / do_SMFFT_CT_DIF / drain; 1: do_SMFFT_CT_DIF_registers (N >= 256); 2: the _wave64 classes (N <= 128).
// nFFTs: whole blocks (a multiple of fft_length / N).  -1: a combination that does not exist.
extern "C" int smfft_example_dif_ct(const void* d_in, void* d_out, int FFT_size, int nFFTs, int inverse, int which, void* stream) {
    const float2* in = (const float2*)d_in;
    float2* out = (float2*)d_out;
    hipStream_t st = (hipStream_t)stream;
    switch (FFT_size) {
        DIF_CASE_SMALL(32) DIF_CASE_SMALL(64) DIF_CASE_SMALL(128) DIF_CASE(256) DIF_CASE(512) DIF_CASE(1024) DIF_CASE(2048) DIF_CASE(4096)
        default: return -1;
    }
}

// The batched circular convolution y = x (*) h of examples/reference_shape_kernel.hip (user_convolution_kernel_registers) with the
// DIF transform in front: the forward transform leaves a thread the bit-reversed positions 4 threadIdx.x + k, which are the
// positions the no-reorder inverse transform takes -- the filter spectrum Hb is given in that same order (Hb = the DIF transform of
// the filter's impulse response, smfft_ct_dif_launch), fetched with the series as one contiguous 32-byte load per thread, and no
// barrier is needed between the two transforms (smfft_dif.hpp).  Against user_convolution_kernel_registers two lines change: the
// forward call and the filter's index.
template <class Fwd, class Inv>
__global__ void __launch_bounds__(Fwd::fft_length_quarter) user_convolution_kernel_dif(const float2* d_x, const float2* d_Hb, float2* d_y) {
    __shared__ float2 s_scratch[Fwd::fft_sm_required];
    constexpr int N = Fwd::fft_length, Q = Fwd::fft_length_quarter;
    const size_t offset = (size_t)blockIdx.x * N;
    float2 x[4], h[4];
    for (int k = 0; k < 4; k++) x[k] = d_x[offset + threadIdx.x + k * Q];
    for (int k = 0; k < 4; k++) h[k] = d_Hb[4 * threadIdx.x + k];
    do_SMFFT_CT_DIF_registers<Fwd>(x, s_scratch);
    for (int k = 0; k < 4; k++) {
        const float2 a = x[k];
        x[k] = make_float2((a.x * h[k].x - a.y * h[k].y) * (1.0f / N), (a.x * h[k].y + a.y * h[k].x) * (1.0f / N));
    }
    do_SMFFT_CT_DIT_registers<Inv>(x, s_scratch);
    for (int k = 0; k < 4; k++) d_y[offset + threadIdx.x + k * Q] = x[k];
}
#define CONV_CASE(N)                                                                                                                            \
    case N:                                                                                                                                     \
        user_convolution_kernel_dif<FFT_##N##_forward_noreorder, FFT_##N##_inverse_noreorder><<<dim3(nSeries), dim3(N / 4), 0, st>>>(x, Hb, y); \
        break;
// d_Hb: N float2, the filter spectrum in bit-reversed order (the DIF transform of the impulse response); N = 256 ... 4096
extern "C" int smfft_example_reference_shape_convolve_dif(const void* d_x, const void* d_Hb, void* d_y, int FFT_size, int nSeries, void* stream) {
    const float2 *x = (const float2*)d_x, *Hb = (const float2*)d_Hb;
    float2* y = (float2*)d_y;
    hipStream_t st = (hipStream_t)stream;
    if (nSeries <= 0) return 0;
    switch (FFT_size) {
        CONV_CASE(256) CONV_CASE(512) CONV_CASE(1024) CONV_CASE(2048) CONV_CASE(4096)
        default: return -1;
    }
    return (int)hipGetLastError();
}

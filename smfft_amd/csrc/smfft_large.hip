// smfft_large.hip -- libsmfft_large.so: the N = 8192 / 16384 single-pass C2C kernels and the C ABI of include/smfft_large.h.
//
// Compiled three times (Makefile): -DSMFFT_LARGE_N=8192 and -DSMFFT_LARGE_N=16384 give one object per length with its kernels and
// its launcher (flags of their own: LARGE_FLAGS_<N>); without SMFFT_LARGE_N it is the C ABI, which only dispatches.
#include <hip/hip_runtime.h>

#include "smfft_large.h"

namespace smfft {
namespace large {
// the persistent grid of N on a device of `cus` compute units: cus x workgroups per CU
template <int N>
int grid(int cus);
// enqueue N-point transforms of nFFTs > 0 FFTs on `stream`, on min(grid<N>(cus), nFFTs) workgroups; 0 or the launch's hipError_t
template <int N>
int launch(const float2* d_input, float2* d_output, int nFFTs, bool inverse, int cus, hipStream_t stream);
}  // namespace large
}  // namespace smfft

#ifdef SMFFT_LARGE_N
#include "smfft/smfft_large.hpp"

namespace smfft {
namespace large {
template <>
int grid<SMFFT_LARGE_N>(int cus) {
    return cus * LargeGeometry<SMFFT_LARGE_N>::kWorkgroupsPerCu;
}

template <>
int launch<SMFFT_LARGE_N>(const float2* d_input, float2* d_output, int nFFTs, bool inverse, int cus, hipStream_t stream) {
    constexpr int N = SMFFT_LARGE_N;
    const int g = grid<N>(cus);
    const dim3 blocks(g < nFFTs ? g : nFFTs), threads(N / 16);
    if (inverse) hipLaunchKernelGGL((large_c2c<N, 1>), blocks, threads, 0, stream, d_input, d_output, nFFTs);
    else hipLaunchKernelGGL((large_c2c<N, 0>), blocks, threads, 0, stream, d_input, d_output, nFFTs);
    return (int)hipGetLastError();
}
}  // namespace large
}  // namespace smfft

#else  // the C ABI
#include "smfft_addon_host.hpp"

namespace {
bool supported(int FFT_size) { return FFT_size == 8192 || FFT_size == 16384; }

int dispatch(const void* d_input, void* d_output, int FFT_size, int nFFTs, int inverse, hipStream_t stream) {
    const int cus = compute_units();
    if (cus <= 0) return (int)hipErrorNoDevice;
    const float2* in = (const float2*)d_input;
    float2* out = (float2*)d_output;
    if (FFT_size == 8192) return smfft::large::launch<8192>(in, out, nFFTs, inverse != 0, cus, stream);
    return smfft::large::launch<16384>(in, out, nFFTs, inverse != 0, cus, stream);
}
}  // namespace

extern "C" {

int smfft_large_launch(const void* d_input, void* d_output, int FFT_size, int nFFTs, int inverse, void* hip_stream) {
    if (!supported(FFT_size) || nFFTs < 0) return -1;
    if (nFFTs == 0) return 0;
    return dispatch(d_input, d_output, FFT_size, nFFTs, inverse, (hipStream_t)hip_stream);
}

int smfft_large_benchmark(const void* d_input, void* d_output, int FFT_size, int nFFTs, int inverse, double* FFT_time) {
    if (!supported(FFT_size) || nFFTs < 0) return -1;
    if (nFFTs == 0) return 0;
    return timed_launch(FFT_time, [&] { return dispatch(d_input, d_output, FFT_size, nFFTs, inverse, nullptr); });
}

int smfft_large_grid(int FFT_size) {
    if (!supported(FFT_size)) return -1;
    const int cus = compute_units();      // 0 when the device cannot be queried, and so is the grid then
    return FFT_size == 8192 ? smfft::large::grid<8192>(cus) : smfft::large::grid<16384>(cus);
}

}  // extern "C"
#endif

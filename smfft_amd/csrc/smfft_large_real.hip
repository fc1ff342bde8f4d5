// smfft_large_real.hip -- libsmfft_large_real.so: the real N = 16384 / 32768 single-pass R2C / C2R kernels and the C ABI of
// include/smfft_large_real.h.
//
// Compiled three times (Makefile): -DSMFFT_LARGE_REAL_N=16384 and -DSMFFT_LARGE_REAL_N=32768 give one object per length with its
// kernels and its launcher (flags of their own: LARGE_REAL_FLAGS_<N>); without SMFFT_LARGE_REAL_N it is the C ABI, which only
// dispatches.
#include <hip/hip_runtime.h>

#include "smfft_large_real.h"

namespace smfft {
namespace large {
// the persistent grid of real N on a device of `cus` compute units: cus x workgroups per CU
template <int N>
int grid_real(int cus);
// enqueue real N-point transforms of nFFTs > 0 FFTs on `stream`, on min(grid_real<N>(cus), nFFTs) workgroups; 0 or the launch's
// hipError_t
template <int N>
int launch_real(const void* d_input, void* d_output, int nFFTs, bool inverse, int cus, hipStream_t stream);
}  // namespace large
}  // namespace smfft

#ifdef SMFFT_LARGE_REAL_N
#include "smfft/smfft_large_real.hpp"

namespace smfft {
namespace large {
template <>
int grid_real<SMFFT_LARGE_REAL_N>(int cus) {
    return cus * LargeRealGeometry<SMFFT_LARGE_REAL_N>::G::kWorkgroupsPerCu;      // (the complex engine of N / 2 points)
}

template <>
int launch_real<SMFFT_LARGE_REAL_N>(const void* d_input, void* d_output, int nFFTs, bool inverse, int cus, hipStream_t stream) {
    constexpr int N = SMFFT_LARGE_REAL_N;
    const int g = grid_real<N>(cus);
    const dim3 blocks(g < nFFTs ? g : nFFTs), threads(N / 32);
    if (inverse) hipLaunchKernelGGL((large_c2r<N>), blocks, threads, 0, stream, (const float2*)d_input, (float*)d_output, nFFTs);
    else hipLaunchKernelGGL((large_r2c<N>), blocks, threads, 0, stream, (const float*)d_input, (float2*)d_output, nFFTs);
    return (int)hipGetLastError();
}
}  // namespace large
}  // namespace smfft

#else  // the C ABI
#include "smfft_addon_host.hpp"

namespace {
bool supported(int FFT_size) { return FFT_size == 16384 || FFT_size == 32768; }

int dispatch(const void* d_input, void* d_output, int FFT_size, int nFFTs, int inverse, hipStream_t stream) {
    const int cus = compute_units();
    if (cus <= 0) return (int)hipErrorNoDevice;
    if (FFT_size == 16384) return smfft::large::launch_real<16384>(d_input, d_output, nFFTs, inverse != 0, cus, stream);
    return smfft::large::launch_real<32768>(d_input, d_output, nFFTs, inverse != 0, cus, stream);
}
}  // namespace

extern "C" {

int smfft_large_real_launch(const void* d_input, void* d_output, int FFT_size, int nFFTs, int inverse, void* hip_stream) {
    if (!supported(FFT_size) || nFFTs < 0) return -1;
    if (nFFTs == 0) return 0;
    return dispatch(d_input, d_output, FFT_size, nFFTs, inverse, (hipStream_t)hip_stream);
}

int smfft_large_real_benchmark(const void* d_input, void* d_output, int FFT_size, int nFFTs, int inverse, double* FFT_time) {
    if (!supported(FFT_size) || nFFTs < 0) return -1;
    if (nFFTs == 0) return 0;
    return timed_launch(FFT_time, [&] { return dispatch(d_input, d_output, FFT_size, nFFTs, inverse, nullptr); });
}

int smfft_large_real_grid(int FFT_size) {
    if (!supported(FFT_size)) return -1;
    const int cus = compute_units();      // 0 when the device cannot be queried, and so is the grid then
    return FFT_size == 16384 ? smfft::large::grid_real<16384>(cus) : smfft::large::grid_real<32768>(cus);
}

}  // extern "C"
#endif

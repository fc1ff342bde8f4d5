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
// enqueue real N-point transforms of nFFTs > 0 FFTs on `stream`; 0 or the launch's hipError_t
template <int N>
int launch_real(const void* d_input, void* d_output, int nFFTs, bool inverse, int grid, hipStream_t stream);
}  // namespace large
}  // namespace smfft

#ifdef SMFFT_LARGE_REAL_N
#include "smfft/smfft_large_real.hpp"

namespace smfft {
namespace large {
template <>
int launch_real<SMFFT_LARGE_REAL_N>(const void* d_input, void* d_output, int nFFTs, bool inverse, int grid, hipStream_t stream) {
    constexpr int N = SMFFT_LARGE_REAL_N;
    const dim3 blocks(grid < nFFTs ? grid : nFFTs), threads(N / 32);
    if (inverse) hipLaunchKernelGGL((large_c2r<N>), blocks, threads, 0, stream, (const float2*)d_input, (float*)d_output, nFFTs);
    else hipLaunchKernelGGL((large_r2c<N>), blocks, threads, 0, stream, (const float*)d_input, (float2*)d_output, nFFTs);
    return (int)hipGetLastError();
}
}  // namespace large
}  // namespace smfft

#else  // the C ABI

namespace {
constexpr int kMaxDevices = 64;
int g_cus[kMaxDevices];     // compute units per device, read once

// the persistent grid of FFT_size on the current device: CUs x workgroups per CU; 0 when the device cannot be queried
int persistent_grid(int FFT_size) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 0;
    int cus = dev < kMaxDevices ? __atomic_load_n(&g_cus[dev], __ATOMIC_RELAXED) : 0;
    if (cus <= 0) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return 0;
        if (dev < kMaxDevices) __atomic_store_n(&g_cus[dev], cus, __ATOMIC_RELAXED);
    }
    return cus * (FFT_size == 16384 ? 2 : 1);
}

bool supported(int FFT_size) { return FFT_size == 16384 || FFT_size == 32768; }

int dispatch(const void* d_input, void* d_output, int FFT_size, int nFFTs, int inverse, hipStream_t stream) {
    const int grid = persistent_grid(FFT_size);
    if (grid <= 0) return (int)hipErrorNoDevice;
    if (FFT_size == 16384) return smfft::large::launch_real<16384>(d_input, d_output, nFFTs, inverse != 0, grid, stream);
    return smfft::large::launch_real<32768>(d_input, d_output, nFFTs, inverse != 0, grid, stream);
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
    hipEvent_t start = nullptr, stop = nullptr;
    int rc = (int)hipEventCreate(&start);
    if (rc == 0) rc = (int)hipEventCreate(&stop);
    if (rc == 0) rc = (int)hipEventRecord(start, nullptr);
    if (rc == 0) rc = dispatch(d_input, d_output, FFT_size, nFFTs, inverse, nullptr);
    if (rc == 0) rc = (int)hipEventRecord(stop, nullptr);
    if (rc == 0) rc = (int)hipEventSynchronize(stop);
    float ms = 0.f;
    if (rc == 0) rc = (int)hipEventElapsedTime(&ms, start, stop);
    if (rc == 0 && FFT_time) *FFT_time += ms;
    if (start) (void)hipEventDestroy(start);
    if (stop) (void)hipEventDestroy(stop);
    return rc;
}

int smfft_large_real_grid(int FFT_size) {
    if (!supported(FFT_size)) return -1;
    return persistent_grid(FFT_size);
}

}  // extern "C"
#endif

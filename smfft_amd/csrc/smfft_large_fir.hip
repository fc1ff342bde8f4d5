// smfft_large_fir.hip -- libsmfft_large_fir.so: the overlap-save FIR filter banks with N = 8192 / 16384 segments and the C ABI of
// include/smfft_large_fir.h.
//
// Compiled three times (Makefile): -DSMFFT_LARGE_FIR_N=8192 and -DSMFFT_LARGE_FIR_N=16384 give one object per length with its kernels
// and its launchers (flags of their own: LARGE_FIR_FLAGS_<N>); without SMFFT_LARGE_FIR_N it is the C ABI, which only checks and
// dispatches (smfft_fir_host.hpp, shared with the banks at N = 256 ... 4096).
//
// The work split (include/smfft/smfft_large_fir.hpp has the two forms of the filter loop; DESIGN.md section 11 the measurement that
// chose between them).  cus = the compute units of the device.
//   * N = 16384, and N = 8192 with one filter: the RECOMPUTE form.  C S K units (segment, filter), filter fastest, on a persistent
//     grid of min(units, cus x workgroups per CU) workgroups.
//   * N = 8192 with K > 1: the HELD form, 25 % faster there.  C S segments x filter groups of
//     smfft::fir_filter_group_size(C S, K, target) filters, target = that form's persistent grid (cus: one workgroup per CU) -- groups
//     = min(K, ceil(cus / (C S))) -- so that a short signal with many filters still fills the chip and a long one pays one forward
//     transform per segment.
// -DSMFFT_LARGE_FIR_HELD_8192=0 (the A/B build of tools/ab_large_fir.py, never the shipped one) keeps N = 8192 on the recompute
// form for every K.
#include <hip/hip_runtime.h>

#include "smfft_fir.hpp"
#include "smfft_large_fir.h"

namespace smfft {
namespace large {
// enqueue on `stream`; cus = compute units of the current device; 0 or the launch's hipError_t
template <int N>
int launch_fir(const float2* x, const float2* H, float2* y, const FirWindow& w, int C, int K, int cus, hipStream_t stream);
template <int N>
int launch_fir_prepare(const float2* taps, int M, int K, int correlate, float2* spectra, int cus, hipStream_t stream);
}  // namespace large
}  // namespace smfft

#ifdef SMFFT_LARGE_FIR_N
#include "smfft/smfft_large_fir.hpp"

#ifndef SMFFT_LARGE_FIR_HELD_8192
#define SMFFT_LARGE_FIR_HELD_8192 1
#endif

namespace smfft {
namespace large {
template <>
int launch_fir<SMFFT_LARGE_FIR_N>(const float2* x, const float2* H, float2* y, const FirWindow& w, int C, int K, int cus, hipStream_t stream) {
    constexpr int N = SMFFT_LARGE_FIR_N;
    const long long segments = w.segments() * C;
#if SMFFT_LARGE_FIR_HELD_8192 && SMFFT_LARGE_FIR_N == 8192
    if (K > 1) {
        const int group = fir_filter_group_size(segments, K, cus);
        const int groups = (K + group - 1) / group;
        const long long units = segments * groups;
        const dim3 blocks((unsigned)(units < cus ? units : cus)), threads(N / 16);
        hipLaunchKernelGGL((large_fir<8192, 1>), blocks, threads, 0, stream, x, H, y, w, K, group, units, large_fir_stride(blocks.x, groups, w.segments()));
        return (int)hipGetLastError();
    }
#endif
    const int grid = cus * LargeGeometry<N>::kWorkgroupsPerCu;
    const long long units = segments * K;
    const dim3 blocks((unsigned)(units < grid ? units : grid)), threads(N / 16);
    hipLaunchKernelGGL((large_fir<N, 0>), blocks, threads, 0, stream, x, H, y, w, K, 1, units, large_fir_stride(blocks.x, K, w.segments()));
    return (int)hipGetLastError();
}

template <>
int launch_fir_prepare<SMFFT_LARGE_FIR_N>(const float2* taps, int M, int K, int correlate, float2* spectra, int cus, hipStream_t stream) {
    constexpr int N = SMFFT_LARGE_FIR_N;
    const int grid = cus * LargeGeometry<N>::kWorkgroupsPerCu;
    const dim3 blocks(K < grid ? K : grid), threads(N / 16);
    hipLaunchKernelGGL((large_fir_prepare<N>), blocks, threads, 0, stream, taps, M, K, correlate, spectra);
    return (int)hipGetLastError();
}
}  // namespace large
}  // namespace smfft

#else  // the C ABI
#include "smfft_fir_host.hpp"

namespace {
struct Bank {
    using Sizes = FirSizes<8192, 16384>;
    template <int N>
    static int launch(const void* x, const smfft::FirWindow& w, int C, const void* H, int K, void* y, hipStream_t stream) {
        const int cus = compute_units();
        if (cus <= 0) return (int)hipErrorNoDevice;
        return smfft::large::launch_fir<N>((const float2*)x, (const float2*)H, (float2*)y, w, C, K, cus, stream);
    }
    template <int N>
    static int launch_prepare(const void* taps, int M, int K, int correlate, void* spectra, hipStream_t stream) {
        const int cus = compute_units();
        if (cus <= 0) return (int)hipErrorNoDevice;
        return smfft::large::launch_fir_prepare<N>((const float2*)taps, M, K, correlate, (float2*)spectra, cus, stream);
    }
};
using Api = FirApi<Bank>;
}  // namespace

extern "C" {

int smfft_large_fir_prepare(const void* d_taps, int n_taps, int n_filters, int FFT_size, int correlate, void* d_spectra, void* hip_stream) {
    return Api::prepare(d_taps, n_taps, n_filters, FFT_size, correlate, d_spectra, hip_stream);
}

int smfft_large_fir_launch(const void* d_signal, long long signal_length, int n_channels, const void* d_spectra, int n_filters, int n_taps,
                           int FFT_size, int correlate, void* d_output, void* hip_stream) {
    return Api::launch(d_signal, signal_length, n_channels, d_spectra, n_filters, n_taps, FFT_size, correlate, d_output, hip_stream);
}

int smfft_large_fir_benchmark(const void* d_signal, long long signal_length, int n_channels, const void* d_spectra, int n_filters, int n_taps,
                              int FFT_size, int correlate, void* d_output, double* FFT_time) {
    return Api::benchmark(d_signal, signal_length, n_channels, d_spectra, n_filters, n_taps, FFT_size, correlate, d_output, FFT_time);
}

}  // extern "C"
#endif

// smfft_fir_detect.hip -- libsmfft_fir_detect.so: the detected outputs of the overlap-save FIR filter banks for complex signals and
// complex taps at N = 256 ... 4096 and the C ABI of include/smfft_fir_detect.h: the power |y|^2 of every filter, or per output sample
// the largest power over the filters and the filter that gave it.
//
// Compiled once per length (Makefile: -DSMFFT_FIR_DETECT_N=256 ... 4096, flags of their own: FIR_DETECT_FLAGS_<N>) for the two kernels
// and their launchers, and once without SMFFT_FIR_DETECT_N for the C ABI, which only checks and dispatches (smfft_fir_host.hpp).
//
// Both kernels are smfft_fir.hip's fir_overlap_save_kernel with another store (the launch constants and the
// power kernel's launcher are smfft_fir_kernel.hpp's, which also says why the bodies are written out in each kernel): the same loads,
// forward transform, product with the prefetched spectrum and inverse transform, and the power of an element is ONE expression,
// __fmaf_rn(re, re, __fmul_rn(im, im)), in both kernels.  The Makefile compiles these objects with -ffp-contract=on, so that the
// transforms of the two kernels fuse the same products into the same sums and the peak is the maximum of the power rows to the bit
// (under the default, fast, the backend chose differently in the two kernels: DESIGN.md section 17).
//   fir_power_kernel<N>   stores that power, one float per element and filter, in the filter loop; the filter-group rule as it is.
//   fir_peak_kernel<N>    one workgroup runs ALL filters of its segments (one filter group, grid.y = 1), keeps the best power and its
//                         filter per element across the filter loop and stores both once per segment, after the loop.
//
// -DSMFFT_FIR_DETECT_WINNERS=0 ... 3: where the peak kernel keeps its sixteen winners per thread (PeakWinners below).  A build variable
// for the A/B of tools/ab_fir_detect.py (a second library beside the shipped one), not a run-time branch; without it every length keeps
// them in registers, which fits the two waves per SIMD of the complex bank at every length.
#include <hip/hip_runtime.h>

#include "smfft_fir.hpp"
#include "smfft_fir_detect.h"

namespace smfft {
namespace fir_detect {
// the peak launch's two outputs behind the one output pointer of smfft_fir_host.hpp's bank
struct PeakOut {
    float* peak;
    int* index;
};
// enqueue on `stream`; 0 or the launch's hipError_t.  Defined per length by the objects compiled with -DSMFFT_FIR_DETECT_N.
template <int N>
int launch_power(const float2* x, const FirWindow& w, int C, const float2* H, int K, float* power, hipStream_t stream);
template <int N>
int launch_peak(const float2* x, const FirWindow& w, int C, const float2* H, int K, float* peak, int* index, hipStream_t stream);
}  // namespace fir_detect
}  // namespace smfft

#ifdef SMFFT_FIR_DETECT_N
#include "smfft_fir_kernel.hpp"

namespace smfft {
namespace fir_detect {

// Where a thread of the peak kernel keeps the best power and the filter index of its sixteen elements across the filter loop.
enum PeakWinners {
    kWinnersRegisters = 0,    // both in registers: 16 + 16 more than the power kernel
    kWinnersLds = 1,          // both in LDS (32 KiB more per workgroup): read, compared and written back every filter
    kWinnersIndexLds = 2,     // the power in registers, the index in LDS (16 KiB more), written only when a filter takes an element
    kWinnersNoPrefetch = 3,   // both in registers, and the filter's spectrum loaded where it is used instead of one filter ahead
};
template <int N>
constexpr int peak_winners_of() {
#ifdef SMFFT_FIR_DETECT_WINNERS
    return SMFFT_FIR_DETECT_WINNERS;
#else
    return kWinnersRegisters;      // at most 243 VGPRs, at N = 4096: two waves per SIMD at every length, so nothing has to move
#endif
}

// the float and int forms of the engine's gstore: one dword per lane, vector memory instructions only
__device__ __forceinline__ void gstore(float* p, float a) { __builtin_nontemporal_store(a, p); }
__device__ __forceinline__ void gstore(int* p, int a) { __builtin_nontemporal_store(a, p); }

// p[(c K + k) L + n] = |y_{c,k}[n]|^2.  The output arrives under the signal's type, the launcher's one Sample (fir_launch), and is
// C K L floats.
template <int N>
__global__ void __launch_bounds__(kFirThreads) fir_power_kernel(const float2* __restrict__ x, const float2* __restrict__ H, float2* __restrict__ y,
                                                                 FirWindow w, int n_channels, int n_filters, int group_size) {
    using G = Geometry<N>;
    __shared__ float2 s[G::kFftsPerBlock * G::SF];
    float* __restrict__ pw = reinterpret_cast<float*>(y);
    Engine<N, 0, 1> fwd;
    Engine<N, 1, 1> inv;
    fwd.init(threadIdx.x);
    inv.init(threadIdx.x);
    float2* sf = s + fwd.fft * G::SF;
    const long long L = w.L, S = w.segments(), total = S * n_channels;
    const long long ntiles = (total + G::kFftsPerBlock - 1) / G::kFftsPerBlock;
    const int k0 = blockIdx.y * group_size;
    const int k1 = min(n_filters, k0 + group_size);
    const int jbegin = w.store_begin();
    // the first filter's spectrum; the filter loop prefetches the next one (after the last filter: the first one for the next tile)
    float2 h[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) h[q] = H[(long long)k0 * N + fwd.u + G::T * q];
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long g = tile * G::kFftsPerBlock + fwd.fft;
        const bool active = g < total;
        const long long c = active ? g / S : 0, seg = active ? g - c * S : 0;
        // x[a + e], zero outside [0, L): a clamped in-range address and a select afterwards, so the 16 loads go out back to back
        const float2* __restrict__ xc = x + c * L;
        const long long a = w.load_start(seg) + fwd.u;
        float2 r[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const long long i = a + G::T * q;
            const long long ic = i < 0 ? 0 : (i < L ? i : L - 1);
            const float2 v = gload(xc + ic);
            r[q] = (i == ic) ? v : make_float2(0.f, 0.f);
        }
        fft_sync<G::kMultiWave>();             // the previous tile's last inverse transform is done with the region
        fwd.transform(r, sf);
        const long long obase = w.output_index(seg, 0);
        const int jend = active ? w.store_end(seg) : 0;
#pragma unroll 1
        for (int k = k0; k < k1; ++k) {
            float2 p[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) p[q] = cmul_fixed(r[q], h[q]);
            const int kn = (k + 1 < k1) ? k + 1 : k0;
#pragma unroll
            for (int q = 0; q < 16; ++q) h[q] = H[(long long)kn * N + fwd.u + G::T * q];
            fft_sync<G::kMultiWave>();         // the forward transform's (or the previous inverse's) last LDS reads are done
            inv.transform(p, sf);
            float* __restrict__ prow = pw + ((c * n_filters + k) * L + obase);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int j = fwd.u + G::T * q;
                if (j >= jbegin && j < jend) gstore(prow + j, __fmaf_rn(p[q].x, p[q].x, __fmul_rn(p[q].y, p[q].y)));
            }
        }
    }
}

// peak[c L + n] = max_k |y_{c,k}[n]|^2, index[c L + n] = the lowest k that attains it; a NaN power is larger than every number and the
// first NaN wins (np.max / np.argmax along the filters).  group_size is n_filters and gridDim.y is 1.
template <int N>
__global__ void __launch_bounds__(kFirThreads) fir_peak_kernel(const float2* __restrict__ x, const float2* __restrict__ H, float* __restrict__ peak,
                                                                int* __restrict__ index, FirWindow w, int n_channels, int n_filters, int group_size) {
    using G = Geometry<N>;
    constexpr int W = peak_winners_of<N>();
    constexpr bool kBestLds = W == kWinnersLds, kIndexLds = W == kWinnersLds || W == kWinnersIndexLds, kPrefetch = W != kWinnersNoPrefetch;
    __shared__ float2 s[G::kFftsPerBlock * G::SF];
    // element q of thread t at [q * 256 + t]: a wave's 64 lanes on 64 consecutive dwords, no bank conflict
    __shared__ float sbest[kBestLds ? 16 * kFirThreads : 1];
    __shared__ int sindex[kIndexLds ? 16 * kFirThreads : 1];
    Engine<N, 0, 1> fwd;
    Engine<N, 1, 1> inv;
    fwd.init(threadIdx.x);
    inv.init(threadIdx.x);
    float2* sf = s + fwd.fft * G::SF;
    const long long L = w.L, S = w.segments(), total = S * n_channels;
    const long long ntiles = (total + G::kFftsPerBlock - 1) / G::kFftsPerBlock;
    const int k0 = blockIdx.y * group_size;
    const int k1 = min(n_filters, k0 + group_size);
    const int jbegin = w.store_begin();
    // the first filter's spectrum; the filter loop prefetches the next one (after the last filter: the first one for the next tile)
    float2 h[16];
    if constexpr (kPrefetch) {
#pragma unroll
        for (int q = 0; q < 16; ++q) h[q] = H[(long long)k0 * N + fwd.u + G::T * q];
    }
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long g = tile * G::kFftsPerBlock + fwd.fft;
        const bool active = g < total;
        const long long c = active ? g / S : 0, seg = active ? g - c * S : 0;
        // x[a + e], zero outside [0, L): a clamped in-range address and a select afterwards, so the 16 loads go out back to back
        const float2* __restrict__ xc = x + c * L;
        const long long a = w.load_start(seg) + fwd.u;
        float2 r[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const long long i = a + G::T * q;
            const long long ic = i < 0 ? 0 : (i < L ? i : L - 1);
            const float2 v = gload(xc + ic);
            r[q] = (i == ic) ? v : make_float2(0.f, 0.f);
        }
        fft_sync<G::kMultiWave>();             // the previous tile's last inverse transform is done with the region
        fwd.transform(r, sf);
        const long long obase = w.output_index(seg, 0);
        const int jend = active ? w.store_end(seg) : 0;
        // the winners so far; the first filter takes every element, whatever these hold (a thread reads and writes its own LDS slots
        // only, so they need no barrier)
        float best[16];
        int arg[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) best[q] = 0.f, arg[q] = 0;
#pragma unroll 1
        for (int k = k0; k < k1; ++k) {
            if constexpr (!kPrefetch) {
#pragma unroll
                for (int q = 0; q < 16; ++q) h[q] = H[(long long)k * N + fwd.u + G::T * q];
            }
            float2 p[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) p[q] = cmul_fixed(r[q], h[q]);
            if constexpr (kPrefetch) {
                const int kn = (k + 1 < k1) ? k + 1 : k0;
#pragma unroll
                for (int q = 0; q < 16; ++q) h[q] = H[(long long)kn * N + fwd.u + G::T * q];
            }
            fft_sync<G::kMultiWave>();         // the forward transform's (or the previous inverse's) last LDS reads are done
            inv.transform(p, sf);
            const bool first = k == k0;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float v = __fmaf_rn(p[q].x, p[q].x, __fmul_rn(p[q].y, p[q].y));
                const float b = kBestLds ? sbest[q * kFirThreads + threadIdx.x] : best[q];
                // take = v > b || (v != v && b == b), or the first filter; without short circuits, which hipcc turns into a branch per element
                const bool take = first | (v > b) | ((v != v) & (b == b));
                if constexpr (kBestLds) {
                    if (take) sbest[q * kFirThreads + threadIdx.x] = v;
                } else {
                    best[q] = take ? v : b;
                }
                if constexpr (kIndexLds) {
                    if (take) sindex[q * kFirThreads + threadIdx.x] = k;
                } else {
                    arg[q] = take ? k : arg[q];
                }
            }
        }
        float* __restrict__ prow = peak + (c * L + obase);
        int* __restrict__ irow = index + (c * L + obase);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int j = fwd.u + G::T * q;
            if (j >= jbegin && j < jend) {
                gstore(prow + j, kBestLds ? sbest[q * kFirThreads + threadIdx.x] : best[q]);
                gstore(irow + j, kIndexLds ? sindex[q * kFirThreads + threadIdx.x] : arg[q]);
            }
        }
    }
}

template <>
int launch_power<SMFFT_FIR_DETECT_N>(const float2* x, const FirWindow& w, int C, const float2* H, int K, float* power, hipStream_t stream) {
    return fir_launch<SMFFT_FIR_DETECT_N>(fir_power_kernel<SMFFT_FIR_DETECT_N>, x, w, w.segments(), C, H, K, reinterpret_cast<float2*>(power), stream);
}

// fir_launch without the filter-group rule: one group of all K filters, so a workgroup sees every filter of its segments
template <>
int launch_peak<SMFFT_FIR_DETECT_N>(const float2* x, const FirWindow& w, int C, const float2* H, int K, float* peak, int* index, hipStream_t stream) {
    constexpr int N = SMFFT_FIR_DETECT_N;
    const long long tiles = (w.segments() * C + Geometry<N>::kFftsPerBlock - 1) / Geometry<N>::kFftsPerBlock;
    const dim3 grid((unsigned)(tiles < kFirGridCap ? tiles : kFirGridCap), 1);
    hipLaunchKernelGGL(fir_peak_kernel<N>, grid, dim3(kFirThreads), 0, stream, x, H, peak, index, w, C, K, K);
    return (int)hipGetLastError();
}

}  // namespace fir_detect
}  // namespace smfft

#else  // the C ABI
#include "smfft_fir_host.hpp"

namespace {
using smfft::fir_detect::PeakOut;
struct PowerBank {
    using Sizes = FirSizes<256, 512, 1024, 2048, 4096>;
    template <int N>
    static int launch(const void* x, const smfft::FirWindow& w, int C, const void* H, int K, void* y, hipStream_t stream) {
        return smfft::fir_detect::launch_power<N>((const float2*)x, w, C, (const float2*)H, K, (float*)y, stream);
    }
};
struct PeakBank {
    using Sizes = PowerBank::Sizes;
    template <int N>
    static int launch(const void* x, const smfft::FirWindow& w, int C, const void* H, int K, void* y, hipStream_t stream) {
        const PeakOut* out = (const PeakOut*)y;
        return smfft::fir_detect::launch_peak<N>((const float2*)x, w, C, (const float2*)H, K, out->peak, out->index, stream);
    }
};
using Power = FirApi<PowerBank>;
using Peak = FirApi<PeakBank>;
}  // namespace

extern "C" {

int smfft_fir_power_launch(const void* d_signal, long long signal_length, int n_channels, const void* d_spectra, int n_filters, int n_taps,
                           int FFT_size, int correlate, void* d_power, void* hip_stream) {
    return Power::launch(d_signal, signal_length, n_channels, d_spectra, n_filters, n_taps, FFT_size, correlate, d_power, hip_stream);
}

int smfft_fir_power_benchmark(const void* d_signal, long long signal_length, int n_channels, const void* d_spectra, int n_filters, int n_taps,
                              int FFT_size, int correlate, void* d_power, double* FFT_time) {
    return Power::benchmark(d_signal, signal_length, n_channels, d_spectra, n_filters, n_taps, FFT_size, correlate, d_power, FFT_time);
}

int smfft_fir_peak_launch(const void* d_signal, long long signal_length, int n_channels, const void* d_spectra, int n_filters, int n_taps,
                          int FFT_size, int correlate, void* d_peak, void* d_index, void* hip_stream) {
    PeakOut out{(float*)d_peak, (int*)d_index};
    return Peak::launch(d_signal, signal_length, n_channels, d_spectra, n_filters, n_taps, FFT_size, correlate, &out, hip_stream);
}

int smfft_fir_peak_benchmark(const void* d_signal, long long signal_length, int n_channels, const void* d_spectra, int n_filters, int n_taps,
                             int FFT_size, int correlate, void* d_peak, void* d_index, double* FFT_time) {
    PeakOut out{(float*)d_peak, (int*)d_index};
    return Peak::benchmark(d_signal, signal_length, n_channels, d_spectra, n_filters, n_taps, FFT_size, correlate, &out, FFT_time);
}

}  // extern "C"
#endif

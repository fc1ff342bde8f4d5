// smfft_fir_real.hip -- libsmfft_fir_real.so: the overlap-save FIR filter banks for real signals and real taps at N = 256 ... 4096 and
// the C ABI of include/smfft_fir_real.h.
//
// Compiled once per length (Makefile: -DSMFFT_FIR_REAL_N=256 ... 4096, flags of their own: FIR_REAL_FLAGS_<N>) for the two kernels
// and their launchers, and once without SMFFT_FIR_REAL_N for the C ABI, which only checks and dispatches.
//
// The kernel is smfft_fir.hip's fir_overlap_save_kernel with another load and another store.  For a real filter
// g, conv(x1 + i x2, g) = conv(x1, g) + i conv(x2, g): two consecutive real segments of a channel go into the real and the imaginary
// lane of one complex transform of the register engine, the product with the filter's ordinary N-point spectrum and the inverse
// transform are those of the complex bank, and the two filtered segments come out in .x and .y.  No Hermitian split or merge, no new
// transform code.  The pairing (pairs per channel, the absent partner of an odd segment count, load starts, store windows) is
// smfft_fir_real.hpp's FirPairs, shared with the host and the CPU test.
//
// -DSMFFT_FIR_REAL_NT_LOADS=0 / 1: the signal loads plain or non-temporal.  A build variable for the A/B of tools/ab_fir_real.py (a
// second library beside the shipped one), not a run-time branch.  Non-temporal loads ship, the complex bank's form: the A/B found
// no difference beyond the run's spread (profiles/r16_fir_real_ab.txt).
#include <hip/hip_runtime.h>

#include "smfft_fir_real.hpp"
#include "smfft_fir_real.h"

namespace smfft {
namespace fir_real {
// enqueue on `stream`; 0 or the launch's hipError_t.  Defined per length by the objects compiled with -DSMFFT_FIR_REAL_N.
template <int N>
int launch(const float* x, const FirPairs& fp, int C, const float2* H, int K, float* y, hipStream_t stream);
template <int N>
int launch_prepare(const float* taps, int M, int K, int correlate, float2* spectra, hipStream_t stream);
}  // namespace fir_real
}  // namespace smfft

#ifdef SMFFT_FIR_REAL_N
#include "smfft/smfft_engine.hpp"

#ifndef SMFFT_FIR_REAL_NT_LOADS
#define SMFFT_FIR_REAL_NT_LOADS 1
#endif

namespace smfft {
namespace fir_real {

constexpr int kFirThreads = 256;
constexpr int kFirGridCap = 12288;          // workgroups along the pair tiles (grid-strided beyond), as smfft_fir.hip
constexpr int kFirTargetWorkgroups = 2048;  // the filter-group rule's target, as smfft_fir.hip

// the float forms of the engine's gload / gstore: one dword per lane, vector memory instructions only
__device__ __forceinline__ float gload(const float* p) {
#if SMFFT_FIR_REAL_NT_LOADS
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}
__device__ __forceinline__ void gstore(float* p, float a) { __builtin_nontemporal_store(a, p); }

template <int N>
__global__ void __launch_bounds__(kFirThreads) fir_real_overlap_save_kernel(const float* __restrict__ x, const float2* __restrict__ H, float* __restrict__ y,
                                                                             FirPairs fp, int n_channels, int n_filters, int group_size) {
    using G = Geometry<N>;
    __shared__ float2 s[G::kFftsPerBlock * G::SF];
    Engine<N, 0, 1> fwd;
    Engine<N, 1, 1> inv;
    fwd.init(threadIdx.x);
    inv.init(threadIdx.x);
    float2* sf = s + fwd.fft * G::SF;
    const long long L = fp.w.L, P = fp.pairs(), total = P * n_channels;
    const long long ntiles = (total + G::kFftsPerBlock - 1) / G::kFftsPerBlock;
    const int V = fp.w.valid();
    const int k0 = blockIdx.y * group_size;
    const int k1 = min(n_filters, k0 + group_size);
    const int jbegin = fp.w.store_begin();
    // the first filter's spectrum; the filter loop prefetches the next one (after the last filter: the first one for the next tile)
    float2 h[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) h[q] = H[(long long)k0 * N + fwd.u + G::T * q];
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long g = tile * G::kFftsPerBlock + fwd.fft;
        const bool active = g < total;
        const long long c = active ? g / P : 0, pair = active ? g - c * P : 0;
        // .x = x[a0 + e], .y = x[a0 + V + e], each zero outside [0, L) and .y zero without a second segment.  Element e of a lane is in
        // range for e in [lo, hi), which is never empty for a present segment (L > s V); an absent one borrows the first lane's
        // addresses.  Every thread loads from a clamped in-range address (one 64-bit base per lane, 32-bit offsets) and zeroes the
        // value afterwards with a bit mask, so the 32 loads are unconditional and go out back to back
        const bool second = fp.present(pair, 1);
        const float* __restrict__ xc = x + c * L;
        const long long a0 = fp.load_start(pair, 0), a1 = second ? fp.load_start(pair, 1) : a0;
        const int lo0 = a0 < 0 ? (int)-a0 : 0, hi0 = L - a0 < N ? (int)(L - a0) : N;
        const int lo1 = a1 < 0 ? (int)-a1 : 0, hi1 = L - a1 < N ? (int)(L - a1) : N;
        // the bases may lie in front of the channel (a < 0) -- they are never dereferenced: only base + clamped element is, always in [0, L)
        const float* __restrict__ x0 = xc + a0;
        const float* __restrict__ x1 = xc + a1;
        const unsigned keep1 = second ? 0xffffffffu : 0u;
        float2 r[16];
        unsigned m0[16], m1[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = fwd.u + G::T * q;
            const int e0 = e < lo0 ? lo0 : (e < hi0 ? e : hi0 - 1);
            const int e1 = e < lo1 ? lo1 : (e < hi1 ? e : hi1 - 1);
            m0[q] = e0 == e ? 0xffffffffu : 0u;
            m1[q] = e1 == e ? keep1 : 0u;
            r[q] = make_float2(gload(x0 + e0), gload(x1 + e1));
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) r[q] = make_float2(__uint_as_float(__float_as_uint(r[q].x) & m0[q]), __uint_as_float(__float_as_uint(r[q].y) & m1[q]));
        fft_sync<G::kMultiWave>();             // the previous tile's last inverse transform is done with the region
        fwd.transform(r, sf);
        const long long obase = fp.output_index(pair, 0, 0);      // the second segment's outputs lie V further on
        const int jend0 = active ? fp.store_end(pair, 0) : 0;
        const int jend1 = active ? fp.store_end(pair, 1) : 0;
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
            float* __restrict__ yrow = y + ((c * n_filters + k) * L + obase);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int j = fwd.u + G::T * q;
                if (j >= jbegin && j < jend0) gstore(yrow + j, p[q].x);
                if (j >= jbegin && j < jend1) gstore(yrow + V + j, p[q].y);
            }
        }
    }
}

// H_k = DFT_N(pad_N(g_k)) / N, natural order, one FFT per filter: g_k = h_k, or g_k[m] = h_k[M - 1 - m] (correlate)
template <int N>
__global__ void __launch_bounds__(kFirThreads) fir_real_prepare_kernel(const float* __restrict__ taps, int M, int n_filters, int correlate, float2* __restrict__ spectra) {
    using G = Geometry<N>;
    __shared__ float2 s[G::kFftsPerBlock * G::SF];
    Engine<N, 0, 1> fwd;
    fwd.init(threadIdx.x);
    const long long k = (long long)blockIdx.x * G::kFftsPerBlock + fwd.fft;
    const bool active = k < n_filters;
    const float* __restrict__ hk = taps + (active ? k : 0) * M;
    float2 r[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int e = fwd.u + G::T * q;
        const bool in = e < M;
        const float t = hk[in ? (correlate ? M - 1 - e : e) : 0];
        r[q] = make_float2(in ? t * (1.0f / N) : 0.f, 0.f);
    }
    fwd.transform(r, s + fwd.fft * G::SF);
    if (active) {
#pragma unroll
        for (int q = 0; q < 16; ++q) spectra[k * N + fwd.u + G::T * q] = r[q];
    }
}

template <>
int launch<SMFFT_FIR_REAL_N>(const float* x, const FirPairs& fp, int C, const float2* H, int K, float* y, hipStream_t stream) {
    constexpr int N = SMFFT_FIR_REAL_N, F = Geometry<N>::kFftsPerBlock;
    const long long tiles = (fp.pairs() * C + F - 1) / F;
    const int group = fir_filter_group_size(tiles, K, kFirTargetWorkgroups);
    const dim3 grid((unsigned)(tiles < kFirGridCap ? tiles : kFirGridCap), (unsigned)((K + group - 1) / group));
    fir_real_overlap_save_kernel<N><<<grid, kFirThreads, 0, stream>>>(x, H, y, fp, C, K, group);
    return (int)hipGetLastError();
}

template <>
int launch_prepare<SMFFT_FIR_REAL_N>(const float* taps, int M, int K, int correlate, float2* spectra, hipStream_t stream) {
    constexpr int N = SMFFT_FIR_REAL_N, F = Geometry<N>::kFftsPerBlock;
    fir_real_prepare_kernel<N><<<(K + F - 1) / F, kFirThreads, 0, stream>>>(taps, M, K, correlate, spectra);
    return (int)hipGetLastError();
}

}  // namespace fir_real
}  // namespace smfft

#else  // the C ABI
#include "smfft_addon_host.hpp"

namespace {
bool supported(int N) { return N == 256 || N == 512 || N == 1024 || N == 2048 || N == 4096; }

// -1: an unsupported combination; 0: launch; 1: nothing to do (an empty signal).  No HIP call.
int check(long long L, int C, int K, int M, int N) {
    if (!supported(N) || M < 1 || M >= N || C <= 0 || K <= 0 || L < 0) return -1;
    return L == 0 ? 1 : 0;
}

int dispatch(const void* x, long long L, int C, const void* H, int K, int M, int N, int correlate, void* y, hipStream_t stream) {
    using namespace smfft::fir_real;
    const smfft::FirPairs fp{smfft::FirWindow{L, N, M, correlate != 0}};
    const float* xs = (const float*)x;
    const float2* hs = (const float2*)H;
    float* ys = (float*)y;
    switch (N) {
        case 256: return launch<256>(xs, fp, C, hs, K, ys, stream);
        case 512: return launch<512>(xs, fp, C, hs, K, ys, stream);
        case 1024: return launch<1024>(xs, fp, C, hs, K, ys, stream);
        case 2048: return launch<2048>(xs, fp, C, hs, K, ys, stream);
        case 4096: return launch<4096>(xs, fp, C, hs, K, ys, stream);
    }
    return -1;
}
}  // namespace

extern "C" {

int smfft_fir_real_prepare(const void* d_taps, int n_taps, int n_filters, int FFT_size, int correlate, void* d_spectra, void* hip_stream) {
    using namespace smfft::fir_real;
    if (!supported(FFT_size) || n_taps < 1 || n_taps >= FFT_size || n_filters <= 0) return -1;
    const float* t = (const float*)d_taps;
    float2* o = (float2*)d_spectra;
    const hipStream_t st = (hipStream_t)hip_stream;
    const int c = correlate != 0;
    switch (FFT_size) {
        case 256: return launch_prepare<256>(t, n_taps, n_filters, c, o, st);
        case 512: return launch_prepare<512>(t, n_taps, n_filters, c, o, st);
        case 1024: return launch_prepare<1024>(t, n_taps, n_filters, c, o, st);
        case 2048: return launch_prepare<2048>(t, n_taps, n_filters, c, o, st);
        case 4096: return launch_prepare<4096>(t, n_taps, n_filters, c, o, st);
    }
    return -1;
}

int smfft_fir_real_launch(const void* d_signal, long long signal_length, int n_channels, const void* d_spectra, int n_filters, int n_taps,
                          int FFT_size, int correlate, void* d_output, void* hip_stream) {
    const int chk = check(signal_length, n_channels, n_filters, n_taps, FFT_size);
    if (chk != 0) return chk < 0 ? -1 : 0;
    return dispatch(d_signal, signal_length, n_channels, d_spectra, n_filters, n_taps, FFT_size, correlate, d_output, (hipStream_t)hip_stream);
}

int smfft_fir_real_benchmark(const void* d_signal, long long signal_length, int n_channels, const void* d_spectra, int n_filters, int n_taps,
                             int FFT_size, int correlate, void* d_output, double* FFT_time) {
    const int chk = check(signal_length, n_channels, n_filters, n_taps, FFT_size);
    if (chk != 0) return chk < 0 ? -1 : 0;
    return timed_launch(FFT_time, [&] { return dispatch(d_signal, signal_length, n_channels, d_spectra, n_filters, n_taps, FFT_size, correlate, d_output, nullptr); });
}

}  // extern "C"
#endif

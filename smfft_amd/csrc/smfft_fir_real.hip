// smfft_fir_real.hip -- libsmfft_fir_real.so: the overlap-save FIR filter banks for real signals and real taps at N = 256 ... 4096 and
// the C ABI of include/smfft_fir_real.h.
//
// Compiled once per length (Makefile: -DSMFFT_FIR_REAL_N=256 ... 4096, flags of their own: FIR_REAL_FLAGS_<N>) for the two kernels
// and their launchers, and once without SMFFT_FIR_REAL_N for the C ABI, which only checks and dispatches (smfft_fir_host.hpp).
//
// The kernel is smfft_fir.hip's fir_overlap_save_kernel with another load and another store (the launch constants
// and the launchers are smfft_fir_kernel.hpp's, which also says why the two bodies are written out twice).  For a real filter g,
// conv(x1 + i x2, g) = conv(x1, g) + i conv(x2, g): two consecutive real segments of a channel go into the real and the imaginary lane of one complex transform of the register engine, the product with the filter's ordinary N-point spectrum and the
// inverse transform are those of the complex bank, and the two filtered segments come out in .x and .y.  No Hermitian split or merge,
// no new transform code.  The pairing (pairs per channel, the absent partner of an odd segment count, load starts, store windows) is
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
#include "smfft_fir_kernel.hpp"

#ifndef SMFFT_FIR_REAL_NT_LOADS
#define SMFFT_FIR_REAL_NT_LOADS 1
#endif

namespace smfft {
namespace fir_real {

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
    return fir_launch<SMFFT_FIR_REAL_N>(fir_real_overlap_save_kernel<SMFFT_FIR_REAL_N>, x, fp, fp.pairs(), C, H, K, y, stream);
}

template <>
int launch_prepare<SMFFT_FIR_REAL_N>(const float* taps, int M, int K, int correlate, float2* spectra, hipStream_t stream) {
    return fir_launch_prepare<SMFFT_FIR_REAL_N>(fir_real_prepare_kernel<SMFFT_FIR_REAL_N>, taps, M, K, correlate, spectra, stream);
}

}  // namespace fir_real
}  // namespace smfft

#else  // the C ABI
#include "smfft_fir_host.hpp"

namespace {
struct Bank {
    using Sizes = FirSizes<256, 512, 1024, 2048, 4096>;
    template <int N>
    static int launch(const void* x, const smfft::FirWindow& w, int C, const void* H, int K, void* y, hipStream_t stream) {
        return smfft::fir_real::launch<N>((const float*)x, smfft::FirPairs{w}, C, (const float2*)H, K, (float*)y, stream);
    }
    template <int N>
    static int launch_prepare(const void* taps, int M, int K, int correlate, void* spectra, hipStream_t stream) {
        return smfft::fir_real::launch_prepare<N>((const float*)taps, M, K, correlate, (float2*)spectra, stream);
    }
};
using Api = FirApi<Bank>;
}  // namespace

extern "C" {

int smfft_fir_real_prepare(const void* d_taps, int n_taps, int n_filters, int FFT_size, int correlate, void* d_spectra, void* hip_stream) {
    return Api::prepare(d_taps, n_taps, n_filters, FFT_size, correlate, d_spectra, hip_stream);
}

int smfft_fir_real_launch(const void* d_signal, long long signal_length, int n_channels, const void* d_spectra, int n_filters, int n_taps,
                          int FFT_size, int correlate, void* d_output, void* hip_stream) {
    return Api::launch(d_signal, signal_length, n_channels, d_spectra, n_filters, n_taps, FFT_size, correlate, d_output, hip_stream);
}

int smfft_fir_real_benchmark(const void* d_signal, long long signal_length, int n_channels, const void* d_spectra, int n_filters, int n_taps,
                             int FFT_size, int correlate, void* d_output, double* FFT_time) {
    return Api::benchmark(d_signal, signal_length, n_channels, d_spectra, n_filters, n_taps, FFT_size, correlate, d_output, FFT_time);
}

}  // extern "C"
#endif

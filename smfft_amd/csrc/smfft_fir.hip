// smfft_fir.hip -- overlap-save FIR filter banks (include/smfft.h, "FIR filter banks"): C channels of a long complex signal, each
// filtered by K filters of M taps, in one kernel from segment load to filtered output.
//
// A workgroup of 256 threads holds 4096 / N segments (the tiled kernels' shape); a segment of any channel is one FFT of the register
// engine smfft::Engine<N, DIR, 1> (the engine of convolve_kernel_registers, examples/fft_convolution.hip: natural order in registers at
// both ends -- r[c] = x[u + T c] in, r[q] = X[u + T q] out -- so the filter spectra are the plain DFT and the store window is an index
// test).  Per segment: one forward transform whose spectrum stays in registers, then for each filter of the workgroup's filter group
// a product with the filter's spectrum, one inverse transform and the predicated store of the segment's valid window.  Every output
// element is written once; nothing but the signal, the spectra (L2-resident) and the outputs touches memory.
// The segmentation (load start, store window, output index) is smfft_fir.hpp's FirWindow, shared with the host and the CPU test.
#include <hip/hip_runtime.h>

#include "smfft/smfft_engine.hpp"
#include "smfft_fir.hpp"
#include "smfft_host_util.hpp"
#include "../../include/smfft.h"

namespace smfft {
namespace {

constexpr int kFirThreads = 256;
constexpr int kFirGridCap = 12288;       // workgroups along the segment tiles (grid-strided beyond), as the external kernels
constexpr int kFirTargetWorkgroups = 2048;  // the filter-group rule's target: twice the workgroups the chip holds at once

template <int N>
__global__ void __launch_bounds__(kFirThreads) fir_overlap_save_kernel(const float2* __restrict__ x, const float2* __restrict__ H, float2* __restrict__ y,
                                                                        FirWindow w, int n_channels, int n_filters, int group_size) {
    using G = Geometry<N>;
    __shared__ float2 s[G::kFftsPerBlock * G::SF];
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
        // x[a + e], zero outside [0, L): every thread loads from a clamped in-range address and selects zero afterwards, so the 16 loads
        // are unconditional and go out back to back (a "load or zero" select makes hipcc branch around each load: smfft_kernels.hpp)
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
            float2* __restrict__ yrow = y + ((c * n_filters + k) * L + obase);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int j = fwd.u + G::T * q;
                if (j >= jbegin && j < jend) gstore(yrow + j, p[q]);
            }
        }
    }
}

// H_k = DFT_N(pad_N(g_k)) / N, natural order, one FFT per filter: g_k = h_k, or g_k[m] = conj(h_k[M - 1 - m]) (correlate)
template <int N>
__global__ void __launch_bounds__(kFirThreads) fir_prepare_kernel(const float2* __restrict__ taps, int M, int n_filters, int correlate, float2* __restrict__ spectra) {
    using G = Geometry<N>;
    __shared__ float2 s[G::kFftsPerBlock * G::SF];
    Engine<N, 0, 1> fwd;
    fwd.init(threadIdx.x);
    const long long k = (long long)blockIdx.x * G::kFftsPerBlock + fwd.fft;
    const bool active = k < n_filters;
    const float2* __restrict__ hk = taps + (active ? k : 0) * M;
    float2 r[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int e = fwd.u + G::T * q;
        const bool in = e < M;
        const float2 t = hk[in ? (correlate ? M - 1 - e : e) : 0];
        const float sy = correlate ? -1.0f / N : 1.0f / N;
        r[q] = in ? make_float2(t.x * (1.0f / N), t.y * sy) : make_float2(0.f, 0.f);
    }
    fwd.transform(r, s + fwd.fft * G::SF);
    if (active) {
#pragma unroll
        for (int q = 0; q < 16; ++q) spectra[k * N + fwd.u + G::T * q] = r[q];
    }
}

bool fir_size_ok(int N) { return N == 256 || N == 512 || N == 1024 || N == 2048 || N == 4096; }

template <int N>
int launch_fir_prepare_n(const float2* taps, int M, int K, int correlate, float2* spectra, hipStream_t st) {
    constexpr int F = Geometry<N>::kFftsPerBlock;
    fir_prepare_kernel<N><<<(K + F - 1) / F, kFirThreads, 0, st>>>(taps, M, K, correlate, spectra);
    return (int)hipGetLastError();
}

template <int N>
int launch_fir_n(const float2* x, const FirWindow& w, int C, const float2* H, int K, float2* y, hipStream_t st) {
    const long long tiles = (w.segments() * C + Geometry<N>::kFftsPerBlock - 1) / Geometry<N>::kFftsPerBlock;
    const int group = fir_filter_group_size(tiles, K, kFirTargetWorkgroups);
    const dim3 grid((unsigned)(tiles < kFirGridCap ? tiles : kFirGridCap), (unsigned)((K + group - 1) / group));
    fir_overlap_save_kernel<N><<<grid, kFirThreads, 0, st>>>(x, H, y, w, C, K, group);
    return (int)hipGetLastError();
}

int dispatch_fir(const void* x, long long L, int C, const void* H, int K, int M, int N, int correlate, void* y, hipStream_t st) {
    const FirWindow w{L, N, M, correlate != 0};
    const float2* xs = (const float2*)x;
    const float2* hs = (const float2*)H;
    float2* ys = (float2*)y;
    switch (N) {
        case 256: return launch_fir_n<256>(xs, w, C, hs, K, ys, st);
        case 512: return launch_fir_n<512>(xs, w, C, hs, K, ys, st);
        case 1024: return launch_fir_n<1024>(xs, w, C, hs, K, ys, st);
        case 2048: return launch_fir_n<2048>(xs, w, C, hs, K, ys, st);
        case 4096: return launch_fir_n<4096>(xs, w, C, hs, K, ys, st);
    }
    return -1;
}

// -1: an unsupported combination; 0: launch; 1: nothing to do (an empty signal).  No HIP call.
int fir_check(long long L, int C, int K, int M, int N) {
    if (!fir_size_ok(N) || M < 1 || M >= N || C <= 0 || K <= 0 || L < 0) return -1;
    return L == 0 ? 1 : 0;
}

}  // namespace
}  // namespace smfft

extern "C" int smfft_fir_prepare(const void* d_taps, int n_taps, int n_filters, int FFT_size, int correlate, void* d_spectra, void* hip_stream) {
    using namespace smfft;
    if (!fir_size_ok(FFT_size) || n_taps < 1 || n_taps >= FFT_size || n_filters <= 0) return -1;
    const float2* t = (const float2*)d_taps;
    float2* o = (float2*)d_spectra;
    const hipStream_t st = (hipStream_t)hip_stream;
    const int c = correlate != 0;
    switch (FFT_size) {
        case 256: return launch_fir_prepare_n<256>(t, n_taps, n_filters, c, o, st);
        case 512: return launch_fir_prepare_n<512>(t, n_taps, n_filters, c, o, st);
        case 1024: return launch_fir_prepare_n<1024>(t, n_taps, n_filters, c, o, st);
        case 2048: return launch_fir_prepare_n<2048>(t, n_taps, n_filters, c, o, st);
        case 4096: return launch_fir_prepare_n<4096>(t, n_taps, n_filters, c, o, st);
    }
    return -1;
}

extern "C" int smfft_fir_launch(const void* d_signal, long long signal_length, int n_channels, const void* d_spectra, int n_filters, int n_taps,
                                int FFT_size, int correlate, void* d_output, void* hip_stream) {
    const int chk = smfft::fir_check(signal_length, n_channels, n_filters, n_taps, FFT_size);
    if (chk != 0) return chk < 0 ? -1 : 0;
    return smfft::dispatch_fir(d_signal, signal_length, n_channels, d_spectra, n_filters, n_taps, FFT_size, correlate, d_output, (hipStream_t)hip_stream);
}

extern "C" int smfft_fir_benchmark(const void* d_signal, long long signal_length, int n_channels, const void* d_spectra, int n_filters, int n_taps,
                                   int FFT_size, int correlate, void* d_output, double* FFT_time) {
    const int chk = smfft::fir_check(signal_length, n_channels, n_filters, n_taps, FFT_size);
    if (chk != 0) return chk < 0 ? -1 : 0;
    GpuTimer timer;
    timer.Start();
    const int rc = smfft::dispatch_fir(d_signal, signal_length, n_channels, d_spectra, n_filters, n_taps, FFT_size, correlate, d_output, 0);
    timer.Stop();
    const float ms = timer.Elapsed();
    if (rc == 0 && FFT_time) *FFT_time += ms;
    return rc;
}

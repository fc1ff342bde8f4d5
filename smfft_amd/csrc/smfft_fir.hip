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
// The launch constants and the launchers are smfft_fir_kernel.hpp's, shared with the real bank (smfft_fir_real.hip); the checks, the
// dispatch over the lengths and the bodies of the three entry points are smfft_fir_host.hpp's, shared with all three banks.
#include <hip/hip_runtime.h>

#include "smfft_fir_kernel.hpp"
#include "smfft_fir_host.hpp"
#include "../../include/smfft.h"

namespace smfft {
namespace {

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

// the bank of smfft_fir_host.hpp
struct Bank {
    using Sizes = FirSizes<256, 512, 1024, 2048, 4096>;
    template <int N>
    static int launch(const void* x, const FirWindow& w, int C, const void* H, int K, void* y, hipStream_t stream) {
        return fir_launch<N>(fir_overlap_save_kernel<N>, (const float2*)x, w, w.segments(), C, (const float2*)H, K, (float2*)y, stream);
    }
    template <int N>
    static int launch_prepare(const void* taps, int M, int K, int correlate, void* spectra, hipStream_t stream) {
        return fir_launch_prepare<N>(fir_prepare_kernel<N>, (const float2*)taps, M, K, correlate, (float2*)spectra, stream);
    }
};
using Api = FirApi<Bank>;

}  // namespace
}  // namespace smfft

extern "C" int smfft_fir_prepare(const void* d_taps, int n_taps, int n_filters, int FFT_size, int correlate, void* d_spectra, void* hip_stream) {
    return smfft::Api::prepare(d_taps, n_taps, n_filters, FFT_size, correlate, d_spectra, hip_stream);
}

extern "C" int smfft_fir_launch(const void* d_signal, long long signal_length, int n_channels, const void* d_spectra, int n_filters, int n_taps,
                                int FFT_size, int correlate, void* d_output, void* hip_stream) {
    return smfft::Api::launch(d_signal, signal_length, n_channels, d_spectra, n_filters, n_taps, FFT_size, correlate, d_output, hip_stream);
}

extern "C" int smfft_fir_benchmark(const void* d_signal, long long signal_length, int n_channels, const void* d_spectra, int n_filters, int n_taps,
                                   int FFT_size, int correlate, void* d_output, double* FFT_time) {
    return smfft::Api::benchmark(d_signal, signal_length, n_channels, d_spectra, n_filters, n_taps, FFT_size, correlate, d_output, FFT_time);
}

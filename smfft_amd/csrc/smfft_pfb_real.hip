// smfft_pfb_real.hip -- libsmfft_pfb_real.so: the critically sampled polyphase filter bank channelizer for REAL streams (weighted sum over
// the P polyphase branches of frames of 2N real samples + the 2N-point real-to-complex transform, in one kernel) and the C ABI of
// include/smfft_pfb_real.h.
//
// Compiled once per length (Makefile: -DSMFFT_PFB_REAL_N=256 ... 4096, flags of their own: PFB_REAL_FLAGS_<N>) for the kernels and their
// launcher, and once without SMFFT_PFB_REAL_N for the C ABI, which only checks and dispatches.
//
// The kernel is smfft_pfb_kernel.hpp's pfb_body -- the loop, the schedule, the transform and the store that both filter banks share --
// on float2 = two consecutive real samples: a frame of 2N reals is N float2, so the plan is smfft::PfbPlan{L / 2, N, P, C} in float2
// units, unchanged.  With the bank below a thread accumulates the PACKED sequence
//     z[n] = w[2n] + i w[2n + 1],   w[m] = sum_p h[2 p N + m] x[(f + p) 2N + m],   n = u + T c
// -- per tap, after the sixteen signal loads, the sixteen coefficient PAIRS (h[2n], h[2n + 1]) as 8-byte loads, then one fused
// multiply-add per component --, and after the transform (r[q] = Z[u + T q]) it splits Z into the spectrum of the real frame X[k],
// 0 <= k < N, with X[N] packed into the imaginary part of element 0 (the layout of the R2C kernels of libsmfft_amd.so).  The split is the
// R2C external kernels' own (smfft_kernels.hpp): HermitianRegisters<N, 0> -- partner values through ds_bpermute, no LDS memory -- for FFTs that live in one wave,
// hermitian_pass's body (hermitian_pass_with: the twiddle handed in) through the FFT's LDS region otherwise; N = 4096 needs W_8192^i,
// which the 4096-entry table does not hold: they are built at compile time from the fp64-rounded octant of W_16384, as smfft_large.hpp
// builds its rows.
//
// -DSMFFT_PFB_REAL_SPLIT=0 / 1: the split through LDS / in registers at every length that can do either (N <= 1024: one wave per FFT).
// -DSMFFT_PFB_REAL_NT_LOADS=0 / 1: the signal loads plain / non-temporal.  Build variables for the A/B of tools/ab_pfb_real.py (a second
// library beside the shipped one), not run-time branches; the defaults are below.
#include <hip/hip_runtime.h>

#include "smfft_pfb.hpp"
#include "smfft_pfb_real.h"

namespace smfft {
namespace pfb_real {
// the bank as the C ABI half sees it (smfft_pfb_host.hpp)
struct Host {
    static constexpr int kSamplesPerElement = 2;       // a float2 of the plan is two real samples: a frame of 2N reals is N float2, L even
    // enqueue on `stream`; plan in float2 units; cus = compute units of the current device; R = the schedule's run length; 0 or the
    // launch's hipError_t.  Defined per length by the objects compiled with -DSMFFT_PFB_REAL_N.
    template <int N>
    static int launch(const void* x, const void* h, void* y, const PfbPlan& plan, int power, long long R, int cus, hipStream_t stream);
};
}  // namespace pfb_real
}  // namespace smfft

#ifdef SMFFT_PFB_REAL_N
#include "smfft_kernels.hpp"
#include "smfft/smfft_large.hpp"
#include "smfft_pfb_kernel.hpp"

#ifndef SMFFT_PFB_REAL_NT_LOADS
#define SMFFT_PFB_REAL_NT_LOADS 1
#endif

namespace smfft {
namespace pfb_real {

// Which split a length uses: the R2C external kernels' measured choice (HermitianRegisters::kEnabled) until tools/ab_pfb_real.py has
// timed both here.
template <int N>
constexpr bool split_in_registers() {
#ifdef SMFFT_PFB_REAL_SPLIT
    return SMFFT_PFB_REAL_SPLIT != 0 && N <= 1024;
#else
    return N == 512 || N == 1024;
#endif
}

// W_{2N}^i, 0 <= i <= N / 2, for the split through LDS: element i * kSplitStep of twiddle_4096 for N <= 2048 -- the values hermitian_pass
// reads --; N = 4096 needs W_8192^i = W_16384^{2i}, built at compile time from the fp64-rounded octant as smfft_large.hpp builds its rows
#if SMFFT_PFB_REAL_N == 4096
struct SplitTwiddles8192 {
    TwiddleValue w[2049];
    constexpr SplitTwiddles8192() : w{} {
        for (int i = 0; i <= 2048; ++i) w[i] = large::w16384(2 * i);
    }
};
static __device__ const SplitTwiddles8192 split_twiddles_8192 = SplitTwiddles8192();
constexpr int kSplitStep = 1;
__device__ __forceinline__ large::GlobalTwiddle* split_twiddles() { return (large::GlobalTwiddle*)split_twiddles_8192.w; }
#else
constexpr int kSplitStep = 4096 / (2 * SMFFT_PFB_REAL_N);
__device__ __forceinline__ large::GlobalTwiddle* split_twiddles() { return (large::GlobalTwiddle*)twiddle_4096; }
#endif

// Z[u + T q] in registers -> X[u + T q] in registers (element 0 = (X[0], X[N])).  sf: the FFT's LDS region, whose last-pass reads may
// still be in flight on entry; on return the next tile's fft_sync orders its re-use.
template <int N>
struct Split {
    using G = Geometry<N>;
    HermitianRegisters<N, 0> herm;
    __device__ __forceinline__ void init(int tid) {
        if constexpr (split_in_registers<N>()) herm.init(tid);
    }
    __device__ __forceinline__ void apply(float2 (&r)[16], float2* sf, const Engine<N, 0, 1>& eng) const {
        if constexpr (split_in_registers<N>()) {
            herm.apply(r);
        } else {
            fft_sync<G::kMultiWave>();             // the last pass's reads are done before the registers are written over them
            eng.store_lds(r, sf);
            fft_sync<G::kMultiWave>();
            // the eight twiddles of a thread are loaded per tile (L1 / L2 hits): their address is hidden from the optimiser, which
            // would otherwise hoist the loop-invariant loads out of the persistent loop into sixteen registers the tap loop needs
            large::GlobalTwiddle* w = split_twiddles();
            asm volatile("" : "+s"(w));
            hermitian_pass_with<N, 0>(sf, eng.u, [w](int i) { return large::twiddle_at<0>(w + i * kSplitStep); });
            fft_sync<G::kMultiWave>();
            eng.load_lds(r, sf);
        }
    }
};

struct Bank {
    using Tap = float2;
    static constexpr int kNtLoads = SMFFT_PFB_REAL_NT_LOADS;
    static constexpr bool kPackedNyquist = true;
    template <int N>
    using Post = Split<N>;
    // the coefficient pairs in two groups of eight: sixteen at once would cost 32 registers beside the 64 of r and v
    template <int T>
    static __device__ __forceinline__ void accumulate(float2 (&r)[16], const float2 (&v)[16], const float2* __restrict__ hp) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            float2 w[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) w[q] = hp[T * (8 * half + q)];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                r[8 * half + q].x = __builtin_fmaf(w[q].x, v[8 * half + q].x, r[8 * half + q].x);
                r[8 * half + q].y = __builtin_fmaf(w[q].y, v[8 * half + q].y, r[8 * half + q].y);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
};

template <int N, int POWER>
__global__ void __launch_bounds__(kPfbThreads) __attribute__((amdgpu_waves_per_eu(3, 3)))
pfb_real_kernel(const float2* __restrict__ x, const float2* __restrict__ h, void* __restrict__ y, PfbPlan plan, long long R) {
    __shared__ float2 s[Geometry<N>::kFftsPerBlock * Geometry<N>::SF];
    pfb_body<N, POWER, Bank>(x, h, y, plan, R, s);
}

template <>
int Host::launch<SMFFT_PFB_REAL_N>(const void* x, const void* h, void* y, const PfbPlan& plan, int power, long long R, int cus, hipStream_t stream) {
    return pfb_launch(pfb_real_kernel<SMFFT_PFB_REAL_N, 0>, pfb_real_kernel<SMFFT_PFB_REAL_N, 1>, (const float2*)x, (const float2*)h, y, plan, power, R, cus, stream);
}

}  // namespace pfb_real
}  // namespace smfft

#else  // the C ABI
#include "smfft_pfb_host.hpp"

using Api = PfbApi<smfft::pfb_real::Host>;

extern "C" {

long long smfft_pfb_real_frames(long long signal_length, int n_channels, int taps_per_channel) { return Api::frames(signal_length, n_channels, taps_per_channel); }

int smfft_pfb_real_default_tile_run(int n_channels, int taps_per_channel) { return Api::default_tile_run_or_error(n_channels, taps_per_channel); }

int smfft_pfb_real_launch_tuned(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                                int power, void* d_output, void* hip_stream, int tile_run) {
    return Api::launch_tuned(d_signal, signal_length, n_streams, d_taps, n_channels, taps_per_channel, power, d_output, hip_stream, tile_run);
}

int smfft_pfb_real_launch(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                          int power, void* d_output, void* hip_stream) {
    return Api::launch_tuned(d_signal, signal_length, n_streams, d_taps, n_channels, taps_per_channel, power, d_output, hip_stream, 0);
}

int smfft_pfb_real_benchmark(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                             int power, void* d_output, double* FFT_time) {
    return Api::benchmark(d_signal, signal_length, n_streams, d_taps, n_channels, taps_per_channel, power, d_output, FFT_time);
}

}  // extern "C"
#endif

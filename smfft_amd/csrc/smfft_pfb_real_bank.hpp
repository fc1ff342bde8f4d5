// smfft_pfb_real_bank.hpp -- the real polyphase filter bank's traits for smfft_pfb_kernel.hpp's loop: per tap the sixteen coefficient
// PAIRS (h[2n], h[2n + 1]) as 8-byte loads and one fused multiply-add per component, and after the transform the Hermitian split of the
// packed spectrum (registers or LDS per length).  Device side only.  Included by smfft_pfb_real.hip (libsmfft_pfb_real.so) and
// smfft_pfb_spec.hip (libsmfft_pfb_spec.so).  The includer defines SMFFT_PFB_REAL_N, the length of the object it compiles (N = 4096
// builds its split's twiddle table), and may define SMFFT_PFB_REAL_SPLIT and SMFFT_PFB_REAL_NT_LOADS (smfft_pfb_real.hip says what
// they are).
#pragma once
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

}  // namespace pfb_real
}  // namespace smfft

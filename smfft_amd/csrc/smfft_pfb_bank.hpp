// smfft_pfb_bank.hpp -- the complex polyphase filter bank's traits for smfft_pfb_kernel.hpp's loop: per tap the sixteen float coefficients
// h[p N + u + T c] after the sixteen signal loads, then two fused multiply-adds per element; nothing between the transform and the
// store.  Device side only.  Included by smfft_pfb.hip (libsmfft_pfb.so) and smfft_pfb_spec.hip (libsmfft_pfb_spec.so), each of which
// may define SMFFT_PFB_NT_LOADS = 0 / 1 first (the signal loads plain / non-temporal; default 1).
#pragma once
#include "smfft_pfb_kernel.hpp"

#ifndef SMFFT_PFB_NT_LOADS
#define SMFFT_PFB_NT_LOADS 1
#endif

namespace smfft {
namespace pfb {

struct Bank {
    using Tap = float;
    static constexpr int kNtLoads = SMFFT_PFB_NT_LOADS;
    static constexpr bool kPackedNyquist = false;
    template <int T>
    static __device__ __forceinline__ void accumulate(float2 (&r)[16], const float2 (&v)[16], const float* __restrict__ hp) {
        float w[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) w[q] = hp[T * q];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            r[q].x = __builtin_fmaf(w[q], v[q].x, r[q].x);
            r[q].y = __builtin_fmaf(w[q], v[q].y, r[q].y);
        }
    }
    template <int N>
    struct Post {
        __device__ __forceinline__ void init(int) {}
        __device__ __forceinline__ void apply(float2 (&)[16], float2*, const Engine<N, 0, 1>&) const {}
    };
};

}  // namespace pfb
}  // namespace smfft

// smfft_large_pfb.hpp -- the polyphase filter bank channelizer for N = 8192 and 16384 channels (gfx950), on the C2C engine of
// smfft_large.hpp: C streams of a long complex signal, a prototype of P N real taps, the weighted sum over the P polyphase branches
// and the N-point forward transform in one kernel from signal load to spectrum store (include/smfft_large_pfb.h; the definition of
// include/smfft_pfb.h at these lengths).
//
// The engine and its geometry are used as they are.  Pass 1 consumes r[c] = x[u + T*c] and pass 4 produces y[q] = X[u + T*q] -- the
// contract of the register engine under pfb_body (smfft_amd/csrc/smfft_pfb_kernel.hpp) -- so the weighted sum is accumulated straight
// into pass 1's input registers and pass 4's output registers are stored as they are.
//
// One (stream, frame) pair is done by one workgroup of T = N / 16 threads, on a persistent grid.  Per pair and thread:
//   * a run-time loop over the taps p, ascending: sixteen unconditional signal loads x[c L + (f + p) N + u + T*q] back to back, then the
//     sixteen coefficients h[p N + u + T*q] (plain loads: shared by every pair, cache resident), then r[q] = fma(h, x, r[q]) per
//     component -- the rounding is written down, so every schedule gives the same bits;
//   * forward passes 1-4 (large_transform: six barriers);
//   * sixteen coalesced non-temporal stores of X[u + T*q], or of fma(re, re, im im) in power mode.
// The index arithmetic of a pair is smfft::PfbPlan (smfft_pfb.hpp), unchanged; which workgroup computes which pair, and when, is
// LargePfbSchedule below.  Both are shared with the host, the CPU tests and tools/large_pfb_model.py.  The pair's two 64-bit offsets are
// uniform and kept in scalar registers; a lane adds one 32-bit offset.
//
// Barriers: the six of the transform.  The tap loop between two transforms touches no LDS, so the engine's sixth barrier still separates
// one pair's read of exchange C from the next pair's write of exchange A.  There is no prefetch of the next pair across it (DESIGN.md
// section 9).
//
// Buffer contract (include/smfft_large_pfb.h): 8-byte-aligned pointers (4 for the taps and the power output), 64-bit element offsets,
// only signal[c L, c L + (F + P - 1) N), taps[0, P N) and out[0, C F N) touched; the three must not overlap.
#pragma once
#include <hip/hip_runtime.h>
#include "smfft_large.hpp"      // LargeEngine, large_transform, uniform, scalar_base, GlobalFloat2
#include "smfft_pfb.hpp"        // smfft::PfbPlan (smfft_amd/csrc)

namespace smfft {
namespace large {

// Which pair workgroup b of a grid of `grid` computes in round t = 0, 1, ...: both forms permute each block of `grid` consecutive
// pairs, so every pair is computed exactly once and its arithmetic does not depend on the form.
//   form 1, stride:       g = t grid + b -- consecutive frames on consecutive workgroups, which the hardware deals round-robin over the
//                         eight XCDs (observed, not a contract): the P frames a pair shares with its neighbours land in eight L2s;
//   form 2, XCD-blocked:  g = t grid + (b mod 8) (grid / 8) + b / 8, grid a multiple of 8 -- the workgroups b = i (mod 8) take grid / 8
//                         consecutive pairs.
struct LargePfbSchedule {
    long long pairs;
    int grid;      // G >= 1 (a multiple of 8 in form 2)
    int form;      // 1 or 2

    // the schedule of a launch: pairs >= 1; cap >= 1 = min(max_workgroups, what the device holds at once); form as asked for (1 or 2)
    __host__ __device__ static LargePfbSchedule make(long long pairs, long long cap, int form) {
        long long g = pairs < cap ? pairs : cap;
        if (form == 2) {
            if (g >= 8) g -= g % 8;
            else form = 1;
        }
        return LargePfbSchedule{pairs, (int)g, form};
    }
    __host__ __device__ long long rounds() const { return (pairs + grid - 1) / grid; }
    // the place of workgroup b in a round's block of `grid` consecutive pairs
    __host__ __device__ int slot(int b) const { return form == 2 ? (b % 8) * (grid / 8) + b / 8 : b; }
    // the pair of workgroup b in round t, or -1 where the last round has none for it
    __host__ __device__ long long pair_of(int b, long long t) const {
        const long long g = t * grid + slot(b);
        return g < pairs ? g : -1;
    }
};

typedef __attribute__((address_space(1))) const float GlobalFloat;
typedef __attribute__((address_space(1))) const v2f GlobalV2f;

// element u of the row at `p` (a scalar base and one 32-bit lane offset), non-temporal (NT) or plain
template <int NT>
__device__ __forceinline__ float2 large_pfb_signal_load(GlobalFloat2* p, unsigned u) {
    if constexpr (NT) {
        const v2f v = __builtin_nontemporal_load((GlobalV2f*)p + u);
        return make_float2(v.x, v.y);
    } else {
        return make_float2(p[u].x, p[u].y);
    }
}

// nothing is scheduled across this point: the sixteen signal loads of a tap stay together and the coefficient loads go out after them
__device__ __forceinline__ void large_pfb_loads_issued() {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_sched_barrier(0);
#endif
}

// ------------------------------------------------------------------------------------------------
// The kernel.  plan in complex samples; sched = LargePfbSchedule::make(plan.pairs(), ...) with sched.grid == gridDim.x.
// NT: the signal loads non-temporal (1) or plain (0) -- the library's build switch.
// ------------------------------------------------------------------------------------------------
template <int N, int POWER, int NT = 0>
__global__ __launch_bounds__(N / 16) __attribute__((amdgpu_waves_per_eu(4)))
void pfb_large(const float2* x, const float* h, void* y, PfbPlan plan, LargePfbSchedule sched) {
    using G = LargeGeometry<N>;
    constexpr int T = G::T;
    __shared__ float2 lds[G::kLdsFloat2];
    LargeEngine<N, 0> fwd(threadIdx.x);
    const unsigned u = threadIdx.x;
    const int P = plan.P;
    // the skip is uniform over the workgroup: all of its threads pass the same barriers
    for (long long t = 0; t * sched.grid < sched.pairs; ++t) {
        const long long g = sched.pair_of((int)blockIdx.x, t);
        if (g < 0) continue;
        GlobalFloat2* xp = (GlobalFloat2*)x + uniform(plan.input_offset(g));
        GlobalFloat* hp = (GlobalFloat*)h;
        float2 r[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) r[q] = make_float2(0.f, 0.f);
#pragma unroll 1
        for (int p = 0; p < P; ++p) {
            float2 v[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) v[q] = large_pfb_signal_load<NT>(scalar_base(xp + T * q), u);
            large_pfb_loads_issued();
            float w[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) w[q] = scalar_base(hp + T * q)[u];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                r[q].x = __builtin_fmaf(w[q], v[q].x, r[q].x);
                r[q].y = __builtin_fmaf(w[q], v[q].y, r[q].y);
            }
            xp += N;
            hp += N;
        }
        fwd.reload_twiddles();
        float2 X[16];
        large_transform<N, 0>(fwd, r, X, lds);
        const long long o = uniform(plan.output_offset(g));
        if constexpr (POWER) {
            float* yo = (float*)y + o + u;
#pragma unroll
            for (int q = 0; q < 16; ++q) __builtin_nontemporal_store(__builtin_fmaf(X[q].x, X[q].x, X[q].y * X[q].y), yo + T * q);
        } else {
            float2* yo = (float2*)y + o + u;
#pragma unroll
            for (int q = 0; q < 16; ++q) gstore(yo + T * q, X[q]);
        }
    }
}

}  // namespace large
}  // namespace smfft

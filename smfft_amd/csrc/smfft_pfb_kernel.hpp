// smfft_pfb_kernel.hpp -- the one kernel body of the polyphase filter banks (smfft_pfb.hip: complex streams, smfft_pfb_real.hip: real
// streams) and their launcher.  Device side only; the C ABI halves share smfft_pfb_host.hpp.
//
// The body has the shape of fir_overlap_save_kernel (smfft_fir.hip): 256 threads hold 4096 / N frames, a frame is one FFT of the
// register engine smfft::Engine<N, 0, 1> (natural order in registers at both ends: r[c] = x[u + T c] in, r[q] = X[u + T q] out).  Per
// tile a thread accumulates its sixteen elements over a run-time loop on the taps p -- per tap sixteen unconditional signal loads back
// to back, then the bank's coefficients (plain loads: shared by every tile, cache resident), then fused multiply-adds with the
// rounding written down --, transforms, lets the bank work on the spectrum, and stores it (or its power) non-temporally.  Slots of a
// partial last tile compute the last valid pair again and skip the store.  All index arithmetic is smfft_pfb.hpp's PfbPlan, shared
// with the host and the CPU tests.
//
// A bank is a traits struct that supplies what the two kernels differ in, and nothing else:
//   Tap                             the coefficient type: float, or float2 = the coefficients of two consecutive real samples
//   kNtLoads                        the signal loads non-temporal (1) or plain (0): the bank's build switch
//   accumulate<T>(r, v, hp)         r[q] += (coefficient at hp[T q]) * v[q], q < 16: loads one tap's coefficients and applies them
//   Post<N>                         init(tid) once per thread; apply(r, sf, eng) between the transform and the store
//   kPackedNyquist                  element 0 of a frame holds two real values (X[0], X[N]): its power is that of X[0] alone
// Each bank's __global__ kernel (its name and attributes are its own) is a wrapper around pfb_body.
#pragma once
#include <hip/hip_runtime.h>

#include "smfft/smfft_engine.hpp"
#include "smfft_pfb.hpp"

namespace smfft {

constexpr int kPfbThreads = 256;
// The persistent grid: what a compute unit holds at once.  Accumulators 32, one tap's samples 32, its coefficients 16 (the complex
// bank's sixteen floats, the real bank's eight pairs at a time), the engine's twiddles and roles, the real bank's register split's
// constants: 131 ... 161 VGPRs in the complex bank, 146 ... 168 in the real one, which is compiled for exactly three waves per SIMD
// (amdgpu_waves_per_eu on its kernel; without it N = 1024 takes 170).  So three waves fit a SIMD, i.e. three workgroups a compute unit
// (LDS, 34 KiB each, would allow four).  tests/test_pfb_cpu.py and tests/test_pfb_real_cpu.py hold the kernels to the 168 VGPRs this
// figure rests on, and to no scratch.
constexpr int kWorkgroupsPerCu = 3;

template <int NT>
__device__ __forceinline__ float2 signal_load(const float2* p) {
    if constexpr (NT) {
        const v2f v = __builtin_nontemporal_load(reinterpret_cast<const v2f*>(p));
        return make_float2(v.x, v.y);
    } else {
        return *p;
    }
}

// s: the workgroup's LDS, Geometry<N>::kFftsPerBlock * Geometry<N>::SF elements
template <int N, int POWER, class Bank>
__device__ __forceinline__ void pfb_body(const float2* __restrict__ x, const typename Bank::Tap* __restrict__ h, void* __restrict__ y, PfbPlan plan,
                                         long long R, float2* s) {
    using G = Geometry<N>;
    Engine<N, 0, 1> eng;
    eng.init(threadIdx.x);
    typename Bank::template Post<N> post;
    post.init(threadIdx.x);
    float2* sf = s + eng.fft * G::SF;
    const long long last = plan.pairs() - 1, runs = plan.runs(R);
    const int P = plan.P;
    for (long long j = blockIdx.x; j < runs; j += gridDim.x) {
        const long long tend = plan.run_end(j, R);
        for (long long tile = plan.run_begin(j, R); tile < tend; ++tile) {
            const long long pair = plan.pair_of(tile, eng.fft);
            const bool active = pair >= 0;
            const long long g = active ? pair : last;     // an inactive slot loads from a valid frame and stores nothing
            const float2* __restrict__ xp = x + plan.input_offset(g) + eng.u;
            const typename Bank::Tap* __restrict__ hp = h + eng.u;
            float2 r[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) r[q] = make_float2(0.f, 0.f);
#pragma unroll 1
            for (int p = 0; p < P; ++p) {
                float2 v[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) v[q] = signal_load<Bank::kNtLoads>(xp + G::T * q);
                __builtin_amdgcn_sched_barrier(0);   // the sixteen signal loads stay together: the coefficient loads go out after them
                Bank::template accumulate<G::T>(r, v, hp);
                xp += N;
                hp += N;
            }
            fft_sync<G::kMultiWave>();             // the previous tile's last LDS reads are done with the region
            eng.transform(r, sf);
            post.apply(r, sf, eng);
            if (active) {
                const long long o = plan.output_offset(g) + eng.u;
                if constexpr (POWER) {
                    float* __restrict__ yo = (float*)y + o;
                    // packed: thread 0's register 0 holds (X[0], X[N]), two real values, and the power of DC alone goes out
                    const float im0 = Bank::kPackedNyquist && eng.u == 0 ? 0.f : r[0].y;
                    __builtin_nontemporal_store(__builtin_fmaf(r[0].x, r[0].x, im0 * im0), yo);
#pragma unroll
                    for (int q = 1; q < 16; ++q) __builtin_nontemporal_store(__builtin_fmaf(r[q].x, r[q].x, r[q].y * r[q].y), yo + G::T * q);
                } else {
                    float2* __restrict__ yo = (float2*)y + o;
#pragma unroll
                    for (int q = 0; q < 16; ++q) gstore(yo + G::T * q, r[q]);
                }
            }
        }
    }
}

// enqueue a bank's kernel pair on `stream`: cus = compute units of the current device; R = the schedule's run length; 0 or the launch's
// hipError_t
template <class Tap, class Kernel>
int pfb_launch(Kernel complex_kernel, Kernel power_kernel, const float2* x, const Tap* h, void* y, const PfbPlan& plan, int power, long long R, int cus,
               hipStream_t stream) {
    const dim3 blocks((unsigned)plan.grid((long long)cus * kWorkgroupsPerCu, R)), threads(kPfbThreads);
    hipLaunchKernelGGL(power ? power_kernel : complex_kernel, blocks, threads, 0, stream, x, h, y, plan, R);
    return (int)hipGetLastError();
}

}  // namespace smfft

// smfft_pfb.hip -- libsmfft_pfb.so: the critically sampled polyphase filter bank channelizer (weighted sum over the P polyphase branches
// + N-point forward FFT, in one kernel) and the C ABI of include/smfft_pfb.h.
//
// Compiled once per length (Makefile: -DSMFFT_PFB_N=256 ... 4096, flags of their own: PFB_FLAGS_<N>) for the kernels and their
// launcher, and once without SMFFT_PFB_N for the C ABI, which only checks and dispatches.
//
// The kernel has the shape of fir_overlap_save_kernel (smfft_fir.hip): 256 threads hold 4096 / N frames, a frame is one FFT of the
// register engine smfft::Engine<N, 0, 1> (natural order in registers at both ends: r[c] = x[u + T c] in, r[q] = X[u + T q] out).  Per
// tile a thread accumulates r[c] = sum_p h[p N + u + T c] x[(f + p) N + u + T c] over a run-time loop on p -- per tap sixteen
// unconditional signal loads back to back, then the sixteen coefficients (plain loads: P N floats <= 512 KiB, shared by every tile,
// cache resident), then two fused multiply-adds per element with the rounding written down -- transforms, and stores the spectrum (or
// its power) non-temporally.  Slots of a partial last tile compute the last valid pair again and skip the store.
// All index arithmetic is smfft_pfb.hpp's PfbPlan, shared with the host and the CPU test.
//
// -DSMFFT_PFB_NT_LOADS=0 / 1: the signal loads plain or non-temporal.  A build variable for the A/B of tools/ab_pfb.py (a second
// library beside the shipped one), not a run-time branch; the default is the library's gload policy until that A/B has been run
// (DESIGN.md section 12).
#include <hip/hip_runtime.h>

#include "smfft_pfb.hpp"
#include "smfft_pfb.h"

namespace smfft {
namespace pfb {
// enqueue on `stream`; cus = compute units of the current device; R = the schedule's run length; 0 or the launch's hipError_t
template <int N>
int launch(const float2* x, const float* h, void* y, const PfbPlan& plan, int power, long long R, int cus, hipStream_t stream);
}  // namespace pfb
}  // namespace smfft

#ifdef SMFFT_PFB_N
#include "smfft/smfft_engine.hpp"

#ifndef SMFFT_PFB_NT_LOADS
#define SMFFT_PFB_NT_LOADS 1
#endif

namespace smfft {
namespace pfb {

constexpr int kThreads = 256;
// The persistent grid: what a compute unit holds at once.  The kernels take 131 ... 161 VGPRs (accumulators 32, one tap's samples 32,
// its coefficients 16, the engine's twiddles and roles), so three waves fit a SIMD, i.e. three workgroups a compute unit (LDS, 34 KiB
// each, would allow four).  tests/test_pfb_cpu.py holds the kernels to the 168 VGPRs this figure rests on.
constexpr int kWorkgroupsPerCu = 3;

__device__ __forceinline__ float2 signal_load(const float2* p) {
#if SMFFT_PFB_NT_LOADS
    const v2f v = __builtin_nontemporal_load(reinterpret_cast<const v2f*>(p));
    return make_float2(v.x, v.y);
#else
    return *p;
#endif
}

template <int N, int POWER>
__global__ void __launch_bounds__(kThreads) pfb_kernel(const float2* __restrict__ x, const float* __restrict__ h, void* __restrict__ y, PfbPlan plan, long long R) {
    using G = Geometry<N>;
    __shared__ float2 s[G::kFftsPerBlock * G::SF];
    Engine<N, 0, 1> eng;
    eng.init(threadIdx.x);
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
            const float* __restrict__ hp = h + eng.u;
            float2 r[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) r[q] = make_float2(0.f, 0.f);
#pragma unroll 1
            for (int p = 0; p < P; ++p) {
                float2 v[16];
                float w[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) v[q] = signal_load(xp + G::T * q);
                __builtin_amdgcn_sched_barrier(0);   // the sixteen signal loads stay together: the coefficient loads go out after them
#pragma unroll
                for (int q = 0; q < 16; ++q) w[q] = hp[G::T * q];
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    r[q].x = __builtin_fmaf(w[q], v[q].x, r[q].x);
                    r[q].y = __builtin_fmaf(w[q], v[q].y, r[q].y);
                }
                xp += N;
                hp += N;
            }
            fft_sync<G::kMultiWave>();             // the previous tile's last LDS reads are done with the region
            eng.transform(r, sf);
            if (active) {
                const long long o = plan.output_offset(g) + eng.u;
                if constexpr (POWER) {
                    float* __restrict__ yo = (float*)y + o;
#pragma unroll
                    for (int q = 0; q < 16; ++q) __builtin_nontemporal_store(__builtin_fmaf(r[q].x, r[q].x, r[q].y * r[q].y), yo + G::T * q);
                } else {
                    float2* __restrict__ yo = (float2*)y + o;
#pragma unroll
                    for (int q = 0; q < 16; ++q) gstore(yo + G::T * q, r[q]);
                }
            }
        }
    }
}

template <>
int launch<SMFFT_PFB_N>(const float2* x, const float* h, void* y, const PfbPlan& plan, int power, long long R, int cus, hipStream_t stream) {
    constexpr int N = SMFFT_PFB_N;
    const dim3 blocks((unsigned)plan.grid((long long)cus * kWorkgroupsPerCu, R)), threads(kThreads);
    if (power) hipLaunchKernelGGL((pfb_kernel<N, 1>), blocks, threads, 0, stream, x, h, y, plan, R);
    else hipLaunchKernelGGL((pfb_kernel<N, 0>), blocks, threads, 0, stream, x, h, y, plan, R);
    return (int)hipGetLastError();
}

}  // namespace pfb
}  // namespace smfft

#else  // the C ABI
#include "smfft_addon_host.hpp"

namespace {
bool supported(int N, int P) { return (N == 256 || N == 512 || N == 1024 || N == 2048 || N == 4096) && P >= 1 && P <= 32; }

// the shipped run length of the schedule: a starting value, the same for every (N, P), until tools/ab_pfb.py has been run on a device
// 
int default_tile_run(int N, int P) {
    (void)N;
    (void)P;
    return 4;
}

// -1: an unsupported combination; 0: launch; 1: nothing to do (no whole frame).  No HIP call.
int check(long long L, int C, int N, int P, int tile_run) {
    if (!supported(N, P) || C <= 0 || L < 0 || tile_run < 0) return -1;
    return smfft::PfbPlan{L, N, P, C}.frames() == 0 ? 1 : 0;
}

int dispatch(const void* x, long long L, int C, const void* h, int N, int P, int power, void* y, int tile_run, hipStream_t stream) {
    const int cus = compute_units();
    if (cus <= 0) return (int)hipErrorNoDevice;
    const smfft::PfbPlan plan{L, N, P, C};
    const long long R = tile_run > 0 ? tile_run : default_tile_run(N, P);
    const float2* xs = (const float2*)x;
    const float* hs = (const float*)h;
    const int pw = power != 0;
    switch (N) {
        case 256: return smfft::pfb::launch<256>(xs, hs, y, plan, pw, R, cus, stream);
        case 512: return smfft::pfb::launch<512>(xs, hs, y, plan, pw, R, cus, stream);
        case 1024: return smfft::pfb::launch<1024>(xs, hs, y, plan, pw, R, cus, stream);
        case 2048: return smfft::pfb::launch<2048>(xs, hs, y, plan, pw, R, cus, stream);
        case 4096: return smfft::pfb::launch<4096>(xs, hs, y, plan, pw, R, cus, stream);
    }
    return -1;
}
}  // namespace

extern "C" {

long long smfft_pfb_frames(long long signal_length, int n_channels, int taps_per_channel) {
    if (!supported(n_channels, taps_per_channel) || signal_length < 0) return -1;
    return smfft::PfbPlan{signal_length, n_channels, taps_per_channel, 1}.frames();
}

int smfft_pfb_default_tile_run(int n_channels, int taps_per_channel) {
    return supported(n_channels, taps_per_channel) ? default_tile_run(n_channels, taps_per_channel) : -1;
}

int smfft_pfb_launch_tuned(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                           int power, void* d_output, void* hip_stream, int tile_run) {
    const int chk = check(signal_length, n_streams, n_channels, taps_per_channel, tile_run);
    if (chk != 0) return chk < 0 ? -1 : 0;
    return dispatch(d_signal, signal_length, n_streams, d_taps, n_channels, taps_per_channel, power, d_output, tile_run, (hipStream_t)hip_stream);
}

int smfft_pfb_launch(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                     int power, void* d_output, void* hip_stream) {
    return smfft_pfb_launch_tuned(d_signal, signal_length, n_streams, d_taps, n_channels, taps_per_channel, power, d_output, hip_stream, 0);
}

int smfft_pfb_benchmark(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                        int power, void* d_output, double* FFT_time) {
    const int chk = check(signal_length, n_streams, n_channels, taps_per_channel, 0);
    if (chk != 0) return chk < 0 ? -1 : 0;
    return timed_launch(FFT_time, [&] { return dispatch(d_signal, signal_length, n_streams, d_taps, n_channels, taps_per_channel, power, d_output, 0, nullptr); });
}

}  // extern "C"
#endif

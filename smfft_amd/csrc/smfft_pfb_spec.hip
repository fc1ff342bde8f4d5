// smfft_pfb_spec.hip -- libsmfft_pfb_spec.so: integrated power spectra of the two critically sampled polyphase filter banks (complex
// streams: smfft_pfb.hip; real streams: smfft_pfb_real.hip) -- per frame the bank's weighted sum over the P polyphase branches, its
// N-point transform and the power of every channel, summed over n_integrate consecutive frames in the thread that computed them --
// and the C ABI of include/smfft_pfb_spec.h.
//
// Compiled once per length (Makefile: -DSMFFT_PFB_SPEC_N=256 ... 4096, flags of their own: PFB_SPEC_FLAGS_<N>) for the kernels of both
// banks and their launchers, and once without SMFFT_PFB_SPEC_N for the C ABI, which only checks and dispatches.
//
// The banks are the shipped ones, not copies: smfft_pfb_bank.hpp and smfft_pfb_real_bank.hpp, with the signal_load of
// smfft_pfb_kernel.hpp.  The loop is this file's own (pfb_spec_body): the work unit is a GROUP (stream c, spectrum i) = T consecutive
// frames of one stream (smfft_pfb_spec.hpp: PfbSpecPlan).  256 threads hold 4096 / N groups; slot j of a tile walks its group's T
// frames, all slots in lockstep (T is the launch's, so every barrier of the engine stays uniform).  Per frame a thread does what
// pfb_body does -- the tap loop with the sixteen signal loads kept together, Bank::accumulate, Engine<N, 0, 1>::transform, Post::apply
// -- then adds its sixteen power values to the group's sums; after frame T - 1 it stores the sixteen sums non-temporally.  Slots of a
// partial last tile compute the last valid group again and store nothing.  The signal is only read: one N-float spectrum goes out per
// T N samples that come in.
//
// -DSMFFT_PFB_SPEC_ACC_LDS=0 / 1: where a thread's sixteen sums live across the tap loop and the transform of the next frame.
//   1  in LDS: 16 KiB beside the engine's 34 KiB, float q of thread t at word 256 q + t (private to the thread, so no barrier; a wave's
//      access to one q is 64 consecutive words: no bank conflict).  The kernels are compiled for three waves per SIMD like the real
//      bank's, and 3 x 51200 B of LDS fit the compute unit's 160 KiB;
//   0  in registers: sixteen more live VGPRs, at whatever occupancy that compiles to (148 ... 184 VGPRs: three workgroups per compute
//      unit in the complex bank up to N = 1024 and in the real one at N = 256, two elsewhere).  The default: with plain signal loads
//      the two forms tie (within 3 %, either sign from run to run), and this one needs no LDS beyond the engine's.
// -DSMFFT_PFB_SPEC_NT_LOADS=0 / 1: the signal loads plain / non-temporal -- the banks' own build switch (SMFFT_PFB_NT_LOADS,
// SMFFT_PFB_REAL_NT_LOADS), set here for both.  A slot walks consecutive frames, so it loads every block of its stream P times in a
// row; the banks' libraries ship non-temporal loads, here plain ones were 1.06 ... 1.36 x faster.
// Build variables for the A/B of tools/ab_pfb_spec.py (a second library beside the shipped one), not run-time branches; the defaults are
// the forms chosen from that measurement (profiles/r15_pfb_spec_ab.txt).  Either way the persistent grid is
// sized by what the device reports for the compiled kernel (hipOccupancyMaxActiveBlocksPerMultiprocessor: its VGPRs and its LDS), not
// by an assumed figure.
#include <hip/hip_runtime.h>

#include "smfft_pfb_spec.hpp"
#include "smfft_pfb_spec.h"

namespace smfft {
namespace pfb_spec {
// a bank as the C ABI half sees it
template <bool REAL>
struct Host {
    static constexpr int kSamplesPerElement = REAL ? 2 : 1;      // a float2 of the plan is one complex sample / two real samples
    // enqueue on `stream`; plan in float2 units; max_workgroups > 0: the grid's cap, 0: what device `dev` with `cus` compute units holds
    // at once; 0 or a hipError_t.  Defined per length by the objects compiled with -DSMFFT_PFB_SPEC_N.
    template <int N>
    static int launch(const void* x, const void* h, void* y, const PfbSpecPlan& plan, int max_workgroups, int dev, int cus, hipStream_t stream);
};
}  // namespace pfb_spec
}  // namespace smfft

#ifdef SMFFT_PFB_SPEC_N
#ifndef SMFFT_PFB_SPEC_NT_LOADS
#define SMFFT_PFB_SPEC_NT_LOADS 0
#endif
#define SMFFT_PFB_NT_LOADS SMFFT_PFB_SPEC_NT_LOADS
#define SMFFT_PFB_REAL_NT_LOADS SMFFT_PFB_SPEC_NT_LOADS
#define SMFFT_PFB_REAL_N SMFFT_PFB_SPEC_N      // the real bank's header builds the split of this object's length
#include "smfft_pfb_bank.hpp"
#include "smfft_pfb_real_bank.hpp"

#ifndef SMFFT_PFB_SPEC_ACC_LDS
#define SMFFT_PFB_SPEC_ACC_LDS 0
#endif
#if SMFFT_PFB_SPEC_ACC_LDS
#define SMFFT_PFB_SPEC_KERNEL __global__ void __launch_bounds__(kPfbThreads) __attribute__((amdgpu_waves_per_eu(3, 3)))
#else
#define SMFFT_PFB_SPEC_KERNEL __global__ void __launch_bounds__(kPfbThreads)
#endif

namespace smfft {
namespace pfb_spec {

constexpr int kAccLds = SMFFT_PFB_SPEC_ACC_LDS;
constexpr int kAccFloats = kAccLds ? 16 * kPfbThreads : 1;

// acc + p with BOTH roundings of the definition: p, the power mode's fmaf(re, re, im * im), is rounded to fp32 before the add.  HIP
// contracts by default, and acc + fmaf(a, a, b * b) may be re-fused into fmaf(a, a, fmaf(b, b, acc)): passing p through an empty asm
// makes it a value the optimiser cannot look into.
__device__ __forceinline__ float add_rounded(float acc, float p) {
    asm volatile("" : "+v"(p));
    return acc + p;
}

// s: the workgroup's LDS of the transform, Geometry<N>::kFftsPerBlock * Geometry<N>::SF elements; a: the thread's sums in LDS (element
// q at a[kPfbThreads * q]), used when kAccLds
template <int N, class Bank>
__device__ __forceinline__ void pfb_spec_body(const float2* __restrict__ x, const typename Bank::Tap* __restrict__ h, float* __restrict__ y, PfbSpecPlan plan,
                                              float2* s, float* a) {
    using G = Geometry<N>;
    Engine<N, 0, 1> eng;
    eng.init(threadIdx.x);
    typename Bank::template Post<N> post;
    post.init(threadIdx.x);
    float2* sf = s + eng.fft * G::SF;
    const long long last = plan.groups() - 1, tiles = plan.tiles();
    const int P = plan.P, T = plan.T;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long group = plan.group_of(tile, eng.fft);
        const bool active = group >= 0;
        const long long g = active ? group : last;        // an inactive slot loads from a valid group and stores nothing
        const float2* __restrict__ xf = x + plan.input_offset(g, 0) + eng.u;      // frame t of the group: + t N
        // the sums start at +0: p is +0, positive or NaN, so 0 + p_0 IS p_0, bit for bit -- the definition's acc = p_0
        float acc[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            if constexpr (kAccLds) a[kPfbThreads * q] = 0.f;
            else acc[q] = 0.f;
        }
#pragma unroll 1
        for (int t = 0; t < T; ++t) {
            const float2* __restrict__ xp = xf;
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
            fft_sync<G::kMultiWave>();             // the previous frame's last LDS reads are done with the region
            eng.transform(r, sf);
            post.apply(r, sf, eng);
            // the power mode's values (smfft_pfb_kernel.hpp).  Packed: thread 0's register 0 holds (X[0], X[N]), two real values, and the
            // power of DC alone is summed
            const float im0 = Bank::kPackedNyquist && eng.u == 0 ? 0.f : r[0].y;
            float pw[16];
            pw[0] = __builtin_fmaf(r[0].x, r[0].x, im0 * im0);
#pragma unroll
            for (int q = 1; q < 16; ++q) pw[q] = __builtin_fmaf(r[q].x, r[q].x, r[q].y * r[q].y);
            if constexpr (kAccLds) {
                float old[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) old[q] = a[kPfbThreads * q];
#pragma unroll
                for (int q = 0; q < 16; ++q) a[kPfbThreads * q] = add_rounded(old[q], pw[q]);
            } else {
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[q] = add_rounded(acc[q], pw[q]);
            }
            xf += N;
        }
        if (active) {
            float* __restrict__ yo = y + plan.output_offset(g) + eng.u;
#pragma unroll
            for (int q = 0; q < 16; ++q) __builtin_nontemporal_store(kAccLds ? a[kPfbThreads * q] : acc[q], yo + G::T * q);
        }
    }
}

template <int N>
SMFFT_PFB_SPEC_KERNEL pfb_spec_kernel(const float2* __restrict__ x, const float* __restrict__ h, float* __restrict__ y, PfbSpecPlan plan) {
    __shared__ float2 s[Geometry<N>::kFftsPerBlock * Geometry<N>::SF];
    __shared__ float a[kAccFloats];
    pfb_spec_body<N, pfb::Bank>(x, h, y, plan, s, a + threadIdx.x % kAccFloats);
}

template <int N>
SMFFT_PFB_SPEC_KERNEL pfb_real_spec_kernel(const float2* __restrict__ x, const float2* __restrict__ h, float* __restrict__ y, PfbSpecPlan plan) {
    __shared__ float2 s[Geometry<N>::kFftsPerBlock * Geometry<N>::SF];
    __shared__ float a[kAccFloats];
    pfb_spec_body<N, pfb_real::Bank>(x, h, y, plan, s, a + threadIdx.x % kAccFloats);
}

// workgroups of `kernel` that one compute unit of device `dev` holds at once, by the compiled kernel's own registers and LDS; asked
// once per device (devices past the cache are asked on every call); 0 when it cannot be found out
template <class Kernel>
int workgroups_per_cu(Kernel kernel, int* cache, int dev) {
    constexpr int kCached = 64;
    int n = dev >= 0 && dev < kCached ? __atomic_load_n(&cache[dev], __ATOMIC_RELAXED) : 0;
    if (n <= 0) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, kPfbThreads, 0) != hipSuccess || n <= 0) return 0;
        if (dev >= 0 && dev < kCached) __atomic_store_n(&cache[dev], n, __ATOMIC_RELAXED);
    }
    return n;
}

template <class Tap, class Kernel>
int spec_launch(Kernel kernel, int* cache, const float2* x, const Tap* h, float* y, const PfbSpecPlan& plan, int max_workgroups, int dev, int cus,
                hipStream_t stream) {
    long long cap = max_workgroups;
    if (cap <= 0) {
        const int per_cu = workgroups_per_cu(kernel, cache, dev);
        if (per_cu <= 0) return (int)hipErrorInvalidDeviceFunction;
        cap = (long long)cus * per_cu;
    }
    const dim3 blocks((unsigned)plan.grid(cap)), threads(kPfbThreads);
    hipLaunchKernelGGL(kernel, blocks, threads, 0, stream, x, h, y, plan);
    return (int)hipGetLastError();
}

static int g_per_cu[2][64];     // [bank][device]: workgroups_per_cu of this length's two kernels

template <>
template <>
int Host<false>::launch<SMFFT_PFB_SPEC_N>(const void* x, const void* h, void* y, const PfbSpecPlan& plan, int max_workgroups, int dev, int cus, hipStream_t stream) {
    return spec_launch(pfb_spec_kernel<SMFFT_PFB_SPEC_N>, g_per_cu[0], (const float2*)x, (const float*)h, (float*)y, plan, max_workgroups, dev, cus, stream);
}

template <>
template <>
int Host<true>::launch<SMFFT_PFB_SPEC_N>(const void* x, const void* h, void* y, const PfbSpecPlan& plan, int max_workgroups, int dev, int cus, hipStream_t stream) {
    return spec_launch(pfb_real_spec_kernel<SMFFT_PFB_SPEC_N>, g_per_cu[1], (const float2*)x, (const float2*)h, (float*)y, plan, max_workgroups, dev, cus, stream);
}

}  // namespace pfb_spec
}  // namespace smfft

#else  // the C ABI
#include "smfft_pfb_host.hpp"

namespace {
// what the eight entry points share, on the banks' predicates and dispatch (smfft_pfb_host.hpp).  All validation happens before any HIP call.
template <bool REAL>
struct SpecApi {
    using Bank = smfft::pfb_spec::Host<REAL>;
    static smfft::PfbSpecPlan plan_of(long long L, int N, int P, int C, int T) { return smfft::PfbSpecPlan{L / Bank::kSamplesPerElement, N, P, C, T}; }

    // -1: an unsupported combination; 0: launch; 1: nothing to do (no whole integration).  No HIP call.
    static int check(long long L, int C, int N, int P, int T, int max_workgroups) {
        if (!pfb_supported(N, P) || T <= 0 || C <= 0 || !pfb_length_ok<Bank>(L) || max_workgroups < 0) return -1;
        return plan_of(L, N, P, C, T).spectra() == 0 ? 1 : 0;
    }

    static long long spectra(long long L, int N, int P, int T) { return pfb_supported(N, P) && T > 0 && pfb_length_ok<Bank>(L) ? plan_of(L, N, P, 1, T).spectra() : -1; }

    static int dispatch(const void* x, long long L, int C, const void* h, int N, int P, int T, void* y, int max_workgroups, hipStream_t stream) {
        const int cus = compute_units();
        int dev = 0;
        if (cus <= 0 || hipGetDevice(&dev) != hipSuccess) return (int)hipErrorNoDevice;
        return pfb_launch_for<Bank>(N, x, h, y, plan_of(L, N, P, C, T), max_workgroups, dev, cus, stream);
    }

    static int launch_tuned(const void* x, long long L, int C, const void* h, int N, int P, int T, void* y, void* hip_stream, int max_workgroups) {
        const int chk = check(L, C, N, P, T, max_workgroups);
        if (chk != 0) return chk < 0 ? -1 : 0;
        return dispatch(x, L, C, h, N, P, T, y, max_workgroups, (hipStream_t)hip_stream);
    }

    static int benchmark(const void* x, long long L, int C, const void* h, int N, int P, int T, void* y, double* FFT_time) {
        const int chk = check(L, C, N, P, T, 0);
        if (chk != 0) return chk < 0 ? -1 : 0;
        return timed_launch(FFT_time, [&] { return dispatch(x, L, C, h, N, P, T, y, 0, nullptr); });
    }
};
using Complex = SpecApi<false>;
using Real = SpecApi<true>;
}  // namespace

extern "C" {

long long smfft_pfb_spec_spectra(long long signal_length, int n_channels, int taps_per_channel, int n_integrate) {
    return Complex::spectra(signal_length, n_channels, taps_per_channel, n_integrate);
}

int smfft_pfb_spec_launch_tuned(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                                int n_integrate, void* d_output, void* hip_stream, int max_workgroups) {
    return Complex::launch_tuned(d_signal, signal_length, n_streams, d_taps, n_channels, taps_per_channel, n_integrate, d_output, hip_stream, max_workgroups);
}

int smfft_pfb_spec_launch(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                          int n_integrate, void* d_output, void* hip_stream) {
    return Complex::launch_tuned(d_signal, signal_length, n_streams, d_taps, n_channels, taps_per_channel, n_integrate, d_output, hip_stream, 0);
}

int smfft_pfb_spec_benchmark(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                             int n_integrate, void* d_output, double* FFT_time) {
    return Complex::benchmark(d_signal, signal_length, n_streams, d_taps, n_channels, taps_per_channel, n_integrate, d_output, FFT_time);
}

long long smfft_pfb_real_spec_spectra(long long signal_length, int n_channels, int taps_per_channel, int n_integrate) {
    return Real::spectra(signal_length, n_channels, taps_per_channel, n_integrate);
}

int smfft_pfb_real_spec_launch_tuned(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                                     int n_integrate, void* d_output, void* hip_stream, int max_workgroups) {
    return Real::launch_tuned(d_signal, signal_length, n_streams, d_taps, n_channels, taps_per_channel, n_integrate, d_output, hip_stream, max_workgroups);
}

int smfft_pfb_real_spec_launch(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                               int n_integrate, void* d_output, void* hip_stream) {
    return Real::launch_tuned(d_signal, signal_length, n_streams, d_taps, n_channels, taps_per_channel, n_integrate, d_output, hip_stream, 0);
}

int smfft_pfb_real_spec_benchmark(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                                  int n_integrate, void* d_output, double* FFT_time) {
    return Real::benchmark(d_signal, signal_length, n_streams, d_taps, n_channels, taps_per_channel, n_integrate, d_output, FFT_time);
}

}  // extern "C"
#endif

// smfft_pfb_real.hip -- libsmfft_pfb_real.so: the critically sampled polyphase filter bank channelizer for REAL streams (weighted sum over
// the P polyphase branches of frames of 2N real samples + the 2N-point real-to-complex transform, in one kernel) and the C ABI of
// include/smfft_pfb_real.h.
//
// Compiled once per length (Makefile: -DSMFFT_PFB_REAL_N=256 ... 4096, flags of their own: PFB_REAL_FLAGS_<N>) for the kernels and their
// launcher, and once without SMFFT_PFB_REAL_N for the C ABI, which only checks and dispatches.
//
// The kernel is pfb_kernel (smfft_pfb.hip) on float2 = two consecutive real samples: a frame of 2N reals is N float2, so the plan is
// smfft::PfbPlan{L / 2, N, P, C} in float2 units, unchanged.  Per tile a thread accumulates the PACKED sequence
//     z[n] = w[2n] + i w[2n + 1],   w[m] = sum_p h[2 p N + m] x[(f + p) 2N + m],   n = u + T c
// -- per tap sixteen unconditional 8-byte signal loads back to back, then the sixteen coefficient PAIRS (h[2n], h[2n + 1]) as 8-byte
// loads, then one fused multiply-add per component --, transforms it with the register engine smfft::Engine<N, 0, 1> (r[q] = Z[u + T q]),
// splits Z into the spectrum of the real frame X[k], 0 <= k < N, with X[N] packed into the imaginary part of element 0 (the layout of
// the R2C kernels of libsmfft_amd.so), and stores it (or its power) non-temporally.  The split is the R2C external kernels' own
// (smfft_kernels.hpp): HermitianRegisters<N, 0> -- partner values through ds_bpermute, no LDS memory -- for FFTs that live in one wave,
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
// enqueue on `stream`; plan in float2 units; cus = compute units of the current device; R = the schedule's run length; 0 or the launch's
// hipError_t
template <int N>
int launch(const float2* x, const float2* h, void* y, const PfbPlan& plan, int power, long long R, int cus, hipStream_t stream);
}  // namespace pfb_real
}  // namespace smfft

#ifdef SMFFT_PFB_REAL_N
#include "smfft_kernels.hpp"
#include "smfft/smfft_large.hpp"

#ifndef SMFFT_PFB_REAL_NT_LOADS
#define SMFFT_PFB_REAL_NT_LOADS 1
#endif

namespace smfft {
namespace pfb_real {

constexpr int kThreads = 256;

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

// The persistent grid: what a compute unit holds at once.  Accumulators 32, one tap's samples 32, eight of its coefficient pairs 16, the
// engine's twiddles and roles, the register split's constants: 146 ... 168 VGPRs with the kernel compiled for exactly three waves per
// SIMD (amdgpu_waves_per_eu below; without it N = 1024 takes 170), i.e. three workgroups a compute unit (LDS, 34 KiB each, would allow
// four).  tests/test_pfb_real_cpu.py holds the kernels to the 168 VGPRs this figure rests on, and to no scratch.
constexpr int kWorkgroupsPerCu = 3;

__device__ __forceinline__ float2 signal_load(const float2* p) {
#if SMFFT_PFB_REAL_NT_LOADS
    const v2f v = __builtin_nontemporal_load(reinterpret_cast<const v2f*>(p));
    return make_float2(v.x, v.y);
#else
    return *p;
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

template <int N, int POWER>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(3, 3)))
pfb_real_kernel(const float2* __restrict__ x, const float2* __restrict__ h, void* __restrict__ y, PfbPlan plan, long long R) {
    using G = Geometry<N>;
    __shared__ float2 s[G::kFftsPerBlock * G::SF];
    Engine<N, 0, 1> eng;
    eng.init(threadIdx.x);
    Split<N> split;
    split.init(threadIdx.x);
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
            const float2* __restrict__ hp = h + eng.u;
            float2 r[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) r[q] = make_float2(0.f, 0.f);
#pragma unroll 1
            for (int p = 0; p < P; ++p) {
                float2 v[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) v[q] = signal_load(xp + G::T * q);
                __builtin_amdgcn_sched_barrier(0);   // the sixteen signal loads stay together: the coefficient loads go out after them
                // the coefficient pairs in two groups of eight: sixteen at once would cost 32 registers beside the 64 of r and v
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    float2 w[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) w[q] = hp[G::T * (8 * half + q)];
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        r[8 * half + q].x = __builtin_fmaf(w[q].x, v[8 * half + q].x, r[8 * half + q].x);
                        r[8 * half + q].y = __builtin_fmaf(w[q].y, v[8 * half + q].y, r[8 * half + q].y);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                xp += N;
                hp += N;
            }
            fft_sync<G::kMultiWave>();             // the previous tile's last LDS reads are done with the region
            eng.transform(r, sf);
            split.apply(r, sf, eng);
            if (active) {
                const long long o = plan.output_offset(g) + eng.u;
                if constexpr (POWER) {
                    float* __restrict__ yo = (float*)y + o;
                    // thread 0's register 0 holds (X[0], X[N]), two real values: the power of DC alone goes out
                    const float im0 = eng.u == 0 ? 0.f : r[0].y;
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

template <>
int launch<SMFFT_PFB_REAL_N>(const float2* x, const float2* h, void* y, const PfbPlan& plan, int power, long long R, int cus, hipStream_t stream) {
    constexpr int N = SMFFT_PFB_REAL_N;
    const dim3 blocks((unsigned)plan.grid((long long)cus * kWorkgroupsPerCu, R)), threads(kThreads);
    if (power) hipLaunchKernelGGL((pfb_real_kernel<N, 1>), blocks, threads, 0, stream, x, h, y, plan, R);
    else hipLaunchKernelGGL((pfb_real_kernel<N, 0>), blocks, threads, 0, stream, x, h, y, plan, R);
    return (int)hipGetLastError();
}

}  // namespace pfb_real
}  // namespace smfft

#else  // the C ABI
#include "smfft_addon_host.hpp"

namespace {
bool supported(int N, int P) { return (N == 256 || N == 512 || N == 1024 || N == 2048 || N == 4096) && P >= 1 && P <= 32; }

// the shipped run length of the schedule: the complex bank's starting value, the same for every (N, P), until tools/ab_pfb_real.py has
// been run on a device
int default_tile_run(int N, int P) {
    (void)N;
    (void)P;
    return 4;
}

// the plan in float2 units: a frame of 2N reals is N float2 (L even)
smfft::PfbPlan plan_of(long long L, int N, int P, int C) { return smfft::PfbPlan{L / 2, N, P, C}; }

// -1: an unsupported combination; 0: launch; 1: nothing to do (no whole frame).  No HIP call.
int check(long long L, int C, int N, int P, int tile_run) {
    if (!supported(N, P) || C <= 0 || L < 0 || (L & 1) || tile_run < 0) return -1;
    return plan_of(L, N, P, C).frames() == 0 ? 1 : 0;
}

int dispatch(const void* x, long long L, int C, const void* h, int N, int P, int power, void* y, int tile_run, hipStream_t stream) {
    const int cus = compute_units();
    if (cus <= 0) return (int)hipErrorNoDevice;
    const smfft::PfbPlan plan = plan_of(L, N, P, C);
    const long long R = tile_run > 0 ? tile_run : default_tile_run(N, P);
    const float2* xs = (const float2*)x;
    const float2* hs = (const float2*)h;
    const int pw = power != 0;
    switch (N) {
        case 256: return smfft::pfb_real::launch<256>(xs, hs, y, plan, pw, R, cus, stream);
        case 512: return smfft::pfb_real::launch<512>(xs, hs, y, plan, pw, R, cus, stream);
        case 1024: return smfft::pfb_real::launch<1024>(xs, hs, y, plan, pw, R, cus, stream);
        case 2048: return smfft::pfb_real::launch<2048>(xs, hs, y, plan, pw, R, cus, stream);
        case 4096: return smfft::pfb_real::launch<4096>(xs, hs, y, plan, pw, R, cus, stream);
    }
    return -1;
}
}  // namespace

extern "C" {

long long smfft_pfb_real_frames(long long signal_length, int n_channels, int taps_per_channel) {
    if (!supported(n_channels, taps_per_channel) || signal_length < 0 || (signal_length & 1)) return -1;
    return plan_of(signal_length, n_channels, taps_per_channel, 1).frames();
}

int smfft_pfb_real_default_tile_run(int n_channels, int taps_per_channel) {
    return supported(n_channels, taps_per_channel) ? default_tile_run(n_channels, taps_per_channel) : -1;
}

int smfft_pfb_real_launch_tuned(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                                int power, void* d_output, void* hip_stream, int tile_run) {
    const int chk = check(signal_length, n_streams, n_channels, taps_per_channel, tile_run);
    if (chk != 0) return chk < 0 ? -1 : 0;
    return dispatch(d_signal, signal_length, n_streams, d_taps, n_channels, taps_per_channel, power, d_output, tile_run, (hipStream_t)hip_stream);
}

int smfft_pfb_real_launch(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                          int power, void* d_output, void* hip_stream) {
    return smfft_pfb_real_launch_tuned(d_signal, signal_length, n_streams, d_taps, n_channels, taps_per_channel, power, d_output, hip_stream, 0);
}

int smfft_pfb_real_benchmark(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                             int power, void* d_output, double* FFT_time) {
    const int chk = check(signal_length, n_streams, n_channels, taps_per_channel, 0);
    if (chk != 0) return chk < 0 ? -1 : 0;
    return timed_launch(FFT_time, [&] { return dispatch(d_signal, signal_length, n_streams, d_taps, n_channels, taps_per_channel, power, d_output, 0, nullptr); });
}

}  // extern "C"
#endif

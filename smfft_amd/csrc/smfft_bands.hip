// smfft_bands.hip -- libsmfft_bands.so: band spectrograms (mel, Bark, octave bands, re-binning) of real signals: the powers of the frames
// of the short-time Fourier transform of smfft_stft.hip (n = 512 ... 8192 samples, powers of two, at any hop) summed along FREQUENCY
// into the bands of a prepared table inside the kernel, in one kernel and one pass through HBM, and the C ABI of include/smfft_bands.h.
//
// Compiled once per M = n / 2 (Makefile: -DSMFFT_BANDS_N=256 ... 4096, flags of their own: BANDS_FLAGS_<M>) for the kernel and its
// launcher, and once without SMFFT_BANDS_N for the C ABI, which checks, builds the plan and dispatches.
//
// The geometry is stft_kernel's (256 threads, 4096 / M transform slots per workgroup, element u + T q in register q, workgroups stride
// over the tiles), and a slot's unit of work is one frame, as there.
// bands_kernel<M>:  per frame the STFT power kernel's values p[k] = re * re + im * im, k <= M, each a statement of its own; behind an
//                   fft_sync they go as floats into the slot's own transform region (M + 1 floats in 17 M / 16 float2), and behind a
//                   second one thread u of the slot serves the bands u, u + T, ...: it reads first, count and offset of its band from the
//                   plan, sums t = w * p -- a statement of its own -- as acc = acc + t in ascending bin order from acc = -0, which
//                   takes the first term as it is, and stores out[(c frames + f) bands + b]: consecutive threads write consecutive
//                   floats.  An empty band stores +0.  The next frame's first fft_sync frees the region.
//                   The plan is copied once per workgroup into LDS behind the transform regions where it fits there (kStageWords words:
//                   79,872 B per workgroup, two workgroups per compute unit) and is read from global memory per frame where it does not.
//
// The frame-to-spectrum step (windowed pairs -> Engine<M, 0, 1> -> partner through LDS -> Hermitian split -> X[k], X[M]) is the
// arithmetic of stft_kernel, statement for statement, written a third time here (smfft_welch.hip has the second copy): smfft_stft.hip
// and smfft_welch.hip are left as they are, because a kernel body moved behind a __device__ function compiles to other code in the
// kernels that ship (smfft_fir_kernel.hpp, DESIGN.md sections 16 and 27).  Under -ffp-contract=on the copies round alike;
// tests/test_sm_bands_gpu.py holds the identity table's output to the bits of the STFT library's powers.  The twiddle row W_n^k is built
// as there, in an object of this library's own.
//
// A/B builds (Makefile; tools/ab_bands.py): -DSMFFT_BANDS_STAGE_PLAN = 1 / 0 the plan copied once per workgroup into LDS behind the
// transform regions where it fits there (kStageWords words) / read from global memory per frame; -DSMFFT_BANDS_NT_LOAD = 1 / 0 the
// sample loads non-temporal / plain.  All builds give the same bits.  The stores are non-temporal (-DSMFFT_BANDS_NT_STORE); the loads
// of the window and of the plan are always plain.
#include <hip/hip_runtime.h>

#include "smfft_bands.h"

namespace smfft {
namespace bands {
// enqueue `grid` workgroups on `stream`; 0 or the launch's hipError_t.  Defined per M by the objects compiled with -DSMFFT_BANDS_N.
template <int M>
int launch_bands(const float* in, float* out, const float* window, const int* plan, int bands, int weights, long long total, long long frames,
                 long long hop, long long stream_stride, int grid, hipStream_t stream);
}  // namespace bands
}  // namespace smfft

#ifdef SMFFT_BANDS_N
#include "smfft_fir_kernel.hpp"
#include "smfft_rows.hpp"

// the policy of the sample loads and of the stores: 1 non-temporal, 0 plain (the STFT's: overlapping frames fetch a sample from HBM
// once and from L2 after that)
#ifndef SMFFT_BANDS_NT_LOAD
#define SMFFT_BANDS_NT_LOAD 0
#endif
#ifndef SMFFT_BANDS_NT_STORE
#define SMFFT_BANDS_NT_STORE SMFFT_NT
#endif
// the plan: 1 copied once per workgroup into LDS behind the transform regions where 3 bands + weights <= kStageWords, 0 read from
// global memory per frame (L1 / L2 serve it).  By measurement (tools/ab_bands.py, profiles/r28_bands_ab.txt):
// staged, the launch takes 0.67 ... 0.90 of the time at all twenty shapes, quartile ranges separate -- a band's weights are read one
// dependent batch after the other, and LDS answers sooner than L1
#ifndef SMFFT_BANDS_STAGE_PLAN
#define SMFFT_BANDS_STAGE_PLAN 1
#endif

namespace smfft {
namespace bands {

using rows::w32768, rows::row_entry, rows::per_tile;

constexpr bool kStagePlan = SMFFT_BANDS_STAGE_PLAN != 0;
// the words of LDS behind the transform regions that a staged plan may take: 34,816 B + 45,056 B = 79,872 B per workgroup, two
// workgroups per compute unit
constexpr int kStageWords = 11264;

// the twiddle row of n = 2 M points as (cos, sin)(2 pi k / n), that is the CONJUGATE of W_n^k (the row of smfft_stft.hip)
template <int M>
struct Rows {
    TwiddleValue wn[M];
    constexpr Rows() : wn{} {
        for (int k = 0; k < M; ++k) wn[k] = w32768(k * (16384 / M));
    }
};
template <int M>
static __device__ const Rows<M> rows = Rows<M>();

// two consecutive floats at 4-byte alignment (samples, window), with the policies above
__device__ __forceinline__ float2 gload2(const float* p) { return rows::gload2<SMFFT_BANDS_NT_LOAD != 0>(p); }
// the window: plain loads, every frame reads it
__device__ __forceinline__ float2 wload2(const float* p) { return rows::gload2<false>(p); }
__device__ __forceinline__ void gstore1(float* p, float v) { rows::gstore1<SMFFT_BANDS_NT_STORE != 0>(p, v); }

// sum_{i < len} wp[i] * pp[i]: every product a statement of its own, the sum in ascending order from -0 -- (-0) + t is t to the bit for
// every t, so one term with weight 1 comes back as it is.  Four terms are loaded at a time; their order in the sum is the bins'
__device__ __forceinline__ float weighted_sum(const float* wp, const float* pp, int len) {
    float acc = -0.f;
    int i = 0;
    for (; i + 4 <= len; i += 4) {
        const float w0 = wp[i], w1 = wp[i + 1], w2 = wp[i + 2], w3 = wp[i + 3];
        const float p0 = pp[i], p1 = pp[i + 1], p2 = pp[i + 2], p3 = pp[i + 3];
        const float t0 = w0 * p0;
        const float t1 = w1 * p1;
        const float t2 = w2 * p2;
        const float t3 = w3 * p3;
        acc = acc + t0;
        acc = acc + t1;
        acc = acc + t2;
        acc = acc + t3;
    }
    for (; i < len; ++i) {
        const float t = wp[i] * pp[i];
        acc = acc + t;
    }
    return acc;
}

// The bands u, u + T, ... of the frame whose M + 1 powers stand in sp, one thread per band: the plan's first[], count[], offset[] at
// tab, its weights at wts (both in global memory, or both in LDS)
template <int T>
__device__ __forceinline__ void sum_bands(const int* tab, const float* wts, const float* sp, int u, int bands, float* yr, bool active) {
    for (int b = u; b < bands; b += T) {
        const int k0 = tab[b], cnt = tab[bands + b], o = tab[2 * bands + b];
        float acc = weighted_sum(wts + o, sp + k0, cnt);
        // an empty band: exactly +0
        acc = cnt > 0 ? acc : 0.f;
        if (active) gstore1(yr + b, acc);
    }
}

// frame g = c frames + f < total reads in[c stream_stride + f hop ... + n), n = 2 M, under window[0, n) (null: all ones):
// out[g bands + b] = sum_i weight[b][i] |X[first[b] + i]|^2 with the plan of smfft_bands_tables at plan (3 bands int32, then `weights`
// floats)
template <int M>
__global__ void __launch_bounds__(kFirThreads) bands_kernel(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ window,
                                                            const int* __restrict__ plan, int bands, int weights, long long total, long long frames,
                                                            long long hop, long long stream_stride) {
    using G = Geometry<M>;
    constexpr int T = G::T;
    __shared__ float2 s[G::kFftsPerBlock * G::SF + (kStagePlan ? kStageWords / 2 : 0)];
    Engine<M, 0, 1> fwd;
    fwd.init(threadIdx.x);
    float2* sf = s + fwd.fft * G::SF;
    const long long ntiles = (total + G::kFftsPerBlock - 1) / G::kFftsPerBlock;
    const bool self = fwd.u == 0;
    // the plan in LDS, where it fits: copied once per workgroup, word for word
    const bool staged = kStagePlan && 3 * bands + weights <= kStageWords;
    int* splan = reinterpret_cast<int*>(s + G::kFftsPerBlock * G::SF);
    if constexpr (kStagePlan) {
        if (staged) {
            for (int i = threadIdx.x; i < 3 * bands + weights; i += kFirThreads) splan[i] = plan[i];
        }
        __syncthreads();
    }
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long g = tile * G::kFftsPerBlock + fwd.fft;
        const bool active = g < total;
        // an inactive slot of the last tile reads frame 0 and stores nothing
        const long long gg = active ? g : 0;
        const long long c = gg / frames;
        const float* xr = in + c * stream_stride + (gg - c * frames) * hop;
        float2 r[16], p[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) r[q] = gload2(xr + 2 * (fwd.u + T * q));
        if (window) {
            float2 w[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) w[q] = wload2(window + 2 * (fwd.u + T * q));
            // nothing is scheduled across this point: the loads all go out before the first arithmetic
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float v0 = r[q].x * w[q].x;
                const float v1 = r[q].y * w[q].y;
                r[q] = make_float2(v0, v1);
            }
        } else {
            __builtin_amdgcn_sched_barrier(0);
        }
        fft_sync<G::kMultiWave>();             // the previous tile's band sums are done with the region
        fwd.transform(r, sf);
        fft_sync<G::kMultiWave>();             // the transform's last LDS reads are done
#pragma unroll
        for (int q = 0; q < 16; ++q) sf[fwd.u + T * q] = r[q];
        fft_sync<G::kMultiWave>();
        // Z[M - (u + T q)] = Z[(T - u) + T (15 - q)]; thread 0's q = 0 reads one element past the data, inside the region's padding: its
        // partner is its own Z[0], put in below
        const float2* partner = sf + (T - fwd.u);
#pragma unroll
        for (int q = 0; q < 16; ++q) p[q] = partner[T * (15 - q)];
        p[0] = self ? r[0] : p[0];
        const int u = per_tile(fwd.u);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float2 w = row_entry(&rows<M>.wn[u + T * q]);        // (c, s): W_n^k = c - i s
            // P = conj p; S = Z + P, D = Z - P; X = S / 2 - (i / 2) (c - i s) D
            const float sx = r[q].x + p[q].x, sy = r[q].y - p[q].y, dx = r[q].x - p[q].x, dy = r[q].y + p[q].y;
            r[q] = make_float2(0.5f * (sx - w.y * dx + w.x * dy), 0.5f * (sy - w.y * dy - w.x * dx));
        }
        // bins 0 and M, both from Z[0] (p[0] holds it): real, with an imaginary part of +0
        const float x0 = p[0].x + p[0].y, xm = p[0].x - p[0].y;
        r[0] = self ? make_float2(x0, 0.f) : r[0];
        // the power kind's values, kept in r[q].x across the barrier
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float pw = r[q].x * r[q].x + r[q].y * r[q].y;
            r[q].x = pw;
        }
        const float pm = xm * xm;              // + 0 * 0
        fft_sync<G::kMultiWave>();             // the partner reads are done with the region
        // the M + 1 powers of the frame as floats in the slot's own region: M + 1 floats in 17 M / 16 float2
        float* sp = reinterpret_cast<float*>(sf);
#pragma unroll
        for (int q = 0; q < 16; ++q) sp[fwd.u + T * q] = r[q].x;
        if (self) sp[M] = pm;
        fft_sync<G::kMultiWave>();
        float* yr = out + g * bands;
        if (staged) {
            sum_bands<T>(splan, reinterpret_cast<const float*>(splan + 3 * bands), sp, fwd.u, bands, yr, active);
        } else {
            sum_bands<T>(plan, reinterpret_cast<const float*>(plan + 3 * bands), sp, fwd.u, bands, yr, active);
        }
    }
}

template <>
int launch_bands<SMFFT_BANDS_N>(const float* in, float* out, const float* window, const int* plan, int bands, int weights, long long total,
                                long long frames, long long hop, long long stream_stride, int grid, hipStream_t stream) {
    hipLaunchKernelGGL(bands_kernel<SMFFT_BANDS_N>, dim3((unsigned)grid), dim3(kFirThreads), 0, stream, in, out, window, plan, bands, weights, total,
                       frames, hop, stream_stride);
    return (int)hipGetLastError();
}

}  // namespace bands
}  // namespace smfft

#else  // the C ABI
#include <vector>

#include "smfft_rows_host.hpp"

namespace {
constexpr unsigned long long kMaxElements = 1ull << 59;      // floats of a buffer: keeps the byte counts below inside 64 bits

auto dispatch(const void* in, void* out, const void* window, const void* plan, int n, int bands, int weights, long long streams, long long frames,
              long long hop, long long stream_stride) {
    return [=](int grid, hipStream_t stream) {
        const int M = half_length_fft_size(n);
        const long long total = streams * frames;
        grid = default_grid(M, total, grid);
        return dispatch_m(M, [&](auto m) {
            return smfft::bands::launch_bands<m()>((const float*)in, (float*)out, (const float*)window, (const int*)plan, bands, weights, total, frames,
                                                   hop, stream_stride, grid, stream);
        });
    };
}

// the words of a plan of `bands` bands and `weights` weights (first[], count[], offset[] as int32, then the weights); -1: refused
long long plan_words(int n, long long bands, long long weights) {
    const int M = half_length_fft_size(n);
    if (M < 0 || bands < 1 || bands > M + 1 || weights < 0 || weights > 4LL * (M + 1)) return -1;
    return 3 * bands + weights;
}

// The plan of a band table into h_plan (null: the check alone); the number of weights, or -1 for a table that breaks a rule of the
// header.  Host only
long long build_plan(int n, int bands, const void* h_first, const void* h_count, const void* h_weights, void* h_plan) {
    const int *first = (const int*)h_first, *count = (const int*)h_count;
    const float* weights = (const float*)h_weights;
    const int M = half_length_fft_size(n);
    if (M < 0 || bands < 1 || bands > M + 1 || !first || !count) return -1;
    long long sum = 0;
    for (int b = 0; b < bands; ++b) {
        if (first[b] < 0 || count[b] < 0 || first[b] > M + 1 || count[b] > M + 1 - first[b]) return -1;
        sum += count[b];
    }
    if (sum > 4LL * (M + 1) || (sum > 0 && !weights)) return -1;
    if (h_plan) {
        int* tab = (int*)h_plan;
        int at = 0;
        for (int b = 0; b < bands; ++b) {
            tab[b] = first[b];
            tab[bands + b] = count[b];
            tab[2 * bands + b] = at;
            at += count[b];
        }
        float* w = (float*)(tab + 3 * bands);
        for (long long i = 0; i < sum; ++i) w[i] = weights[i];
    }
    return sum;
}

// -1: refused; 0: launch; 1: nothing to do.  No HIP call.  The output overlaps neither the range of the frames, nor the window, nor the
// plan's plan_bytes
int check(const void* in, const void* out, const void* window, const void* plan, int n, int bands, int weights, long long streams, long long frames,
          long long hop, long long stream_stride) {
    const int M = half_length_fft_size(n);
    const long long words = plan_words(n, bands, weights);
    if (M < 0 || words < 0 || !plan || streams < 0 || frames < 0 || hop < 1 || stream_stride < 1) return -1;
    if (streams == 0 || frames == 0) return 1;
    // the 2^59 rule of smfft_stft.hip's check, in 128 bits
    const unsigned __int128 total = (unsigned __int128)streams * (unsigned __int128)frames;
    const unsigned __int128 extent = (unsigned __int128)(streams - 1) * (unsigned __int128)stream_stride
                                     + (unsigned __int128)(frames - 1) * (unsigned __int128)hop + (unsigned)n;
    if (total > kMaxElements / (unsigned)n || extent > kMaxElements) return -1;
    // floats of the output: `bands` sums per frame, bands <= M + 1
    const unsigned long long outs = (unsigned long long)total * (unsigned)bands;
    if (overlap(in, (unsigned long long)extent, out, outs)) return -1;
    if (window && overlap(window, (unsigned)n, out, outs)) return -1;
    if (overlap(plan, (unsigned long long)words, out, outs)) return -1;
    return 0;
}
}  // namespace

extern "C" {

int smfft_bands_fft_size(int n) { return half_length_fft_size(n); }

long long smfft_bands_frames(long long L, int n, long long hop) {
    if (half_length_fft_size(n) < 0 || hop < 1 || L < 0) return -1;
    return L < n ? 0 : 1 + (L - n) / hop;
}

long long smfft_bands_plan_bytes(int n, int bands, int weights) {
    const long long words = plan_words(n, bands, weights);
    return words < 0 ? -1 : 4 * words;
}

int smfft_bands_tables(int n, int bands, const void* h_first, const void* h_count, const void* h_weights, void* h_plan) {
    if (!h_plan) return -1;
    return build_plan(n, bands, h_first, h_count, h_weights, h_plan) < 0 ? -1 : 0;
}

int smfft_bands_prepare(int n, int bands, const void* h_first, const void* h_count, const void* h_weights, void* d_plan, void* hip_stream) {
    const long long sum = build_plan(n, bands, h_first, h_count, h_weights, nullptr);
    if (sum < 0 || !d_plan) return -1;
    std::vector<int> plan(3 * (size_t)bands + (size_t)sum);
    build_plan(n, bands, h_first, h_count, h_weights, plan.data());
    int rc = (int)hipMemcpyAsync(d_plan, plan.data(), plan.size() * sizeof(int), hipMemcpyHostToDevice, (hipStream_t)hip_stream);
    if (rc == 0) rc = (int)hipStreamSynchronize((hipStream_t)hip_stream);      // the host copy of the plan ends with this call
    return rc;
}

int smfft_bands_launch(const void* d_in, void* d_out, const void* d_window, const void* d_plan, int n, int bands, int weights, long long streams, long long frames, long long hop, long long stream_stride, void* hip_stream) {
    return checked_launch(check(d_in, d_out, d_window, d_plan, n, bands, weights, streams, frames, hop, stream_stride),
                          dispatch(d_in, d_out, d_window, d_plan, n, bands, weights, streams, frames, hop, stream_stride), hip_stream);
}

int smfft_bands_launch_tuned(const void* d_in, void* d_out, const void* d_window, const void* d_plan, int n, int bands, int weights, long long streams, long long frames, long long hop, long long stream_stride, void* hip_stream, int grid) {
    return checked_launch_tuned(check(d_in, d_out, d_window, d_plan, n, bands, weights, streams, frames, hop, stream_stride),
                                dispatch(d_in, d_out, d_window, d_plan, n, bands, weights, streams, frames, hop, stream_stride), hip_stream, grid);
}

int smfft_bands_benchmark(const void* d_in, void* d_out, const void* d_window, const void* d_plan, int n, int bands, int weights, long long streams, long long frames, long long hop, long long stream_stride, double* FFT_time) {
    return checked_benchmark(check(d_in, d_out, d_window, d_plan, n, bands, weights, streams, frames, hop, stream_stride),
                             dispatch(d_in, d_out, d_window, d_plan, n, bands, weights, streams, frames, hop, stream_stride), FFT_time);
}

}  // extern "C"
#endif

// smfft_welch.hip -- libsmfft_welch.so: Welch power spectra and cross spectra of real signals, the frames of the short-time Fourier
// transform of smfft_stft.hip (n = 512 ... 8192 samples, powers of two, at any hop) summed over T consecutive frames inside the kernel,
// as |X|^2 of one signal or as conj(X) Y of two, in one kernel and one pass through HBM, and the C ABI of include/smfft_welch.h.
//
// Compiled once per M = n / 2 (Makefile: -DSMFFT_WELCH_N=256 ... 4096, flags of their own: WELCH_FLAGS_<M>) for the two kernels and
// their launchers, and once without SMFFT_WELCH_N for the C ABI, which checks and dispatches.
//
// The geometry is stft_kernel's (256 threads, 4096 / M transform slots per workgroup, element u + T q in register q, workgroups stride
// over the tiles), but a slot's unit of work is one (stream, group), not one frame: the slot loops over the frames of its group and
// keeps the running sums of its sixteen bins -- thread u = 0 also that of bin M -- on chip, and stores them once behind the loop: in
// registers, but for the cross kernel from M = 512 on, which keeps them in LDS (SMFFT_WELCH_CSD_ACC_LDS below).
// welch_kernel<M>:  per frame the STFT power kernel's value p = re * re + im * im, a statement of its own, and acc = acc + p from
//                   acc = -0, which takes p_0 as it is: the sequential fp32 sum in frame order of what stft_kernel<M, 1> stores.
// csd_kernel<M>:    per frame X from x's frame, kept in registers, then Y from y's frame through the same LDS region, then
//                   re = xr * yr + xi * yi (the one expression of the power kernel), a = xr * yi, b = xi * yr, im = a - b, and the same
//                   sums per component.  Bins 0 and M are real in X and in Y: their imaginary parts are stored as +0.
//
// The frame-to-spectrum step (windowed pairs -> Engine<M, 0, 1> -> partner through LDS -> Hermitian split -> X[k], X[M]) is the
// arithmetic of stft_kernel, statement for statement, written a second time here (frame_spectrum): smfft_stft.hip is left as it is,
// because a kernel body moved behind a __device__ function compiles to other code in the kernels that ship (smfft_fir_kernel.hpp,
// DESIGN.md sections 16 and 27).  Under -ffp-contract=on the two copies round alike; tests/test_sm_welch_gpu.py holds the sums to the
// bits of the STFT library's powers.  The twiddle row W_n^k is built as there, in an object of this library's own.
//
// A/B builds (Makefile; tools/ab_welch.py): -DSMFFT_WELCH_NT_LOAD = 1 / 0 the sample loads non-temporal / plain,
// -DSMFFT_WELCH_KEEP_WINDOW / -DSMFFT_WELCH_CSD_KEEP_WINDOW = 1 / 0 the window in registers across the frames of a group / loaded
// again per frame (auto / cross kernel),
// -DSMFFT_WELCH_PREFETCH = 1 / 0 the next frame's sample loads issued in front of the current frame's transform / behind it.  All
// builds give the same bits.  The stores are non-temporal (-DSMFFT_WELCH_NT_STORE); the window's loads are always plain.
#include <hip/hip_runtime.h>

#include "smfft_welch.h"

namespace smfft {
namespace welch {
// enqueue `grid` workgroups on `stream`; 0 or the launch's hipError_t.  Defined per M by the objects compiled with -DSMFFT_WELCH_N.
template <int M>
int launch_welch(const float* in, float* out, const float* window, long long total, long long groups, long long count, long long hop,
                 long long stream_stride, int grid, hipStream_t stream);
template <int M>
int launch_csd(const float* x, const float* y, float2* out, const float* window, long long total, long long groups, long long count, long long hop,
               long long x_stride, long long y_stride, int grid, hipStream_t stream);
}  // namespace welch
}  // namespace smfft

#ifdef SMFFT_WELCH_N
#include "smfft_fir_kernel.hpp"
#include "smfft_rows.hpp"

// the policy of the sample loads and of the stores: 1 non-temporal, 0 plain
#ifndef SMFFT_WELCH_NT_LOAD
#define SMFFT_WELCH_NT_LOAD 0
#endif
#ifndef SMFFT_WELCH_NT_STORE
#define SMFFT_WELCH_NT_STORE SMFFT_NT
#endif
// the window: 1 in registers across the frames of a group, 0 loaded again per frame; per kernel and per M by measurement
// (tools/ab_welch.py, profiles/r27_welch_ab.txt).  With the window kept, the auto kernel takes 1.03 ... 1.28
// times as long at M = 256 and from M = 512 on ties or takes less (down to 0.60 of the time at M = 4096, T = 64); the cross kernel
// takes 0.84 ... 0.93 of the time at M = 512 and 1024 and 1.16 ... 1.32 times as long at M = 256, 2048 and 4096; at M = 1024 it needs
// 88 B of scratch for that, so of the two it ships at M = 512 alone.  The Makefile's WELCH_KEEP_WINDOW sets both
#ifndef SMFFT_WELCH_KEEP_WINDOW
#define SMFFT_WELCH_KEEP_WINDOW (SMFFT_WELCH_N >= 512)
#endif
#ifndef SMFFT_WELCH_CSD_KEEP_WINDOW
#define SMFFT_WELCH_CSD_KEEP_WINDOW (SMFFT_WELCH_N == 512)
#endif
// the next frame's sample loads: 1 in front of the current frame's transform, 0 behind it
#ifndef SMFFT_WELCH_PREFETCH
#define SMFFT_WELCH_PREFETCH 0
#endif
// the cross kernel's thirty-two sums of a thread: 0 in registers, 1 in LDS behind the transform regions (16 x 256 float2 = 32,768 B:
// 67,584 B per workgroup, two workgroups per compute unit).  In registers the kernel fits the 256 VGPRs of two waves per SIMD at
// M = 256 alone and spills 28 ... 128 B of scratch from M = 512 on; with the sums in LDS it takes 240 ... 253 and no scratch there
#ifndef SMFFT_WELCH_CSD_ACC_LDS
#define SMFFT_WELCH_CSD_ACC_LDS (SMFFT_WELCH_N > 256)
#endif

namespace smfft {
namespace welch {

using rows::w32768, rows::row_entry, rows::per_tile;

constexpr bool kKeepWindowAuto = SMFFT_WELCH_KEEP_WINDOW != 0, kKeepWindowCross = SMFFT_WELCH_CSD_KEEP_WINDOW != 0;
constexpr bool kPrefetch = SMFFT_WELCH_PREFETCH != 0;
constexpr bool kAccLds = SMFFT_WELCH_CSD_ACC_LDS != 0;

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

__device__ __forceinline__ void gstore1(float* p, float v) { rows::gstore1<SMFFT_WELCH_NT_STORE != 0>(p, v); }
__device__ __forceinline__ void gstorec(float2* p, float a, float b) { rows::gstorec<SMFFT_WELCH_NT_STORE != 0>(p, a, b); }

// the sixteen pairs of a thread of the frame at p, with the policy above; of the window: plain loads, every frame reads it
template <int M>
__device__ __forceinline__ void load_pairs(const float* p, int u, float2 (&r)[16]) {
#pragma unroll
    for (int q = 0; q < 16; ++q) r[q] = rows::gload2<SMFFT_WELCH_NT_LOAD != 0>(p + 2 * (u + Geometry<M>::T * q));
}
template <int M>
__device__ __forceinline__ void load_window(const float* p, int u, float2 (&w)[16]) {
#pragma unroll
    for (int q = 0; q < 16; ++q) w[q] = rows::gload2<false>(p + 2 * (u + Geometry<M>::T * q));
}
// the windowed samples: products of their own statement, as in stft_kernel
__device__ __forceinline__ void apply_window(float2 (&r)[16], const float2 (&w)[16]) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const float v0 = r[q].x * w[q].x;
        const float v1 = r[q].y * w[q].y;
        r[q] = make_float2(v0, v1);
    }
}

// The windowed pairs of a frame in r -> X[u + T q] in r[q], X[M] (real) in xm; thread 0's r[0] is (X[0], +0).  The statements of
// stft_kernel from its first fft_sync to its r[0], in their order.  The region sf is free again after the next fft_sync.
template <int M>
__device__ __forceinline__ void frame_spectrum(const Engine<M, 0, 1>& fwd, float2* sf, float2 (&r)[16], float& xm, bool self) {
    using G = Geometry<M>;
    constexpr int T = G::T;
    float2 p[16];
    fft_sync<G::kMultiWave>();             // the previous frame's partner reads are done with the region
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
    const float x0 = p[0].x + p[0].y;
    xm = p[0].x - p[0].y;
    r[0] = self ? make_float2(x0, 0.f) : r[0];
}

// group g = c groups + j < total sums the frames j count ... j count + count - 1 of stream c, frame f at in[c stream_stride + f hop ... + n),
// n = 2 M, under window[0, n) (null: all ones): out[g (M + 1) + k] = sum_t |X_t[k]|^2, k <= M, in frame order
template <int M>
__global__ void __launch_bounds__(kFirThreads) __attribute__((amdgpu_waves_per_eu(2))) welch_kernel(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ window,
                                                            long long total, long long groups, long long count, long long hop, long long stream_stride) {
    using G = Geometry<M>;
    constexpr int T = G::T;
    __shared__ float2 s[G::kFftsPerBlock * G::SF];
    Engine<M, 0, 1> fwd;
    fwd.init(threadIdx.x);
    float2* sf = s + fwd.fft * G::SF;
    const long long ntiles = (total + G::kFftsPerBlock - 1) / G::kFftsPerBlock;
    const bool self = fwd.u == 0;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        // (one slot per workgroup at M = 4096: the group and its pointers are the workgroup's, scalars)
        const long long g = G::kFftsPerBlock == 1 ? tile : tile * G::kFftsPerBlock + fwd.fft;
        const bool active = g < total;
        // an inactive slot of the last tile reads group 0 and stores nothing
        const long long gg = active ? g : 0;
        const long long c = gg / groups;
        const float* xr = in + c * stream_stride + (gg - c * groups) * count * hop;
        // the sums start at -0: (-0) + p is p to the bit for every p, so the first frame's term is taken as it is (acc = p_0)
        float acc[16], accm = -0.f;
        float2 r[16], nx[16], w[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = -0.f;
        if (kKeepWindowAuto && window) load_window<M>(window, fwd.u, w);
        if (kPrefetch) load_pairs<M>(xr, fwd.u, nx);
        for (long long t = 0; t < count; ++t) {
            if constexpr (kPrefetch) {
#pragma unroll
                for (int q = 0; q < 16; ++q) r[q] = nx[q];
            } else {
                load_pairs<M>(xr + t * hop, fwd.u, r);
            }
            if (window) {
                if (!kKeepWindowAuto) load_window<M>(window, per_tile(fwd.u), w);   // per_tile: loaded here, not hoisted and kept
                // nothing is scheduled across this point: the loads all go out before the first arithmetic
                __builtin_amdgcn_sched_barrier(0);
                apply_window(r, w);
            } else {
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (kPrefetch) {
                // the next frame's samples, in flight during this frame's transform
                if (t + 1 < count) load_pairs<M>(xr + (t + 1) * hop, fwd.u, nx);
                __builtin_amdgcn_sched_barrier(0);
            }
            float xm;
            frame_spectrum<M>(fwd, sf, r, xm, self);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float pw = r[q].x * r[q].x + r[q].y * r[q].y;
                acc[q] = acc[q] + pw;
            }
            const float pm = xm * xm;          // + 0 * 0
            accm = accm + pm;
        }
        float* yr = out + g * (M + 1);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            if (active) gstore1(yr + (fwd.u + T * q), acc[q]);
        }
        if (active && self) gstore1(yr + M, accm);
    }
}

// the same groups of x and of y (stream c of y at y + c y_stride; y_stride = 0: one reference stream):
// out[g (M + 1) + k] = sum_t conj(X_t[k]) Y_t[k], k <= M, in frame order
template <int M>
__global__ void __launch_bounds__(kFirThreads) __attribute__((amdgpu_waves_per_eu(2))) csd_kernel(const float* x, const float* y, float2* __restrict__ out, const float* __restrict__ window,
                                                          long long total, long long groups, long long count, long long hop, long long x_stride,
                                                          long long y_stride) {
    using G = Geometry<M>;
    constexpr int T = G::T;
    __shared__ float2 s[G::kFftsPerBlock * G::SF + (kAccLds ? 16 * kFirThreads : 0)];
    Engine<M, 0, 1> fwd;
    fwd.init(threadIdx.x);
    float2* sf = s + fwd.fft * G::SF;
    const long long ntiles = (total + G::kFftsPerBlock - 1) / G::kFftsPerBlock;
    const bool self = fwd.u == 0;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        // (one slot per workgroup at M = 4096: the group and its pointers are the workgroup's, scalars)
        const long long g = G::kFftsPerBlock == 1 ? tile : tile * G::kFftsPerBlock + fwd.fft;
        const bool active = g < total;
        // an inactive slot of the last tile reads group 0 and stores nothing
        const long long gg = active ? g : 0;
        const long long c = gg / groups;
        const long long first_sample = (gg - c * groups) * count * hop;
        const float* xr = x + c * x_stride + first_sample;
        const float* yr = y + c * y_stride + first_sample;
        float2 acc[16], xs[16], r[16], nx[16], w[16];
        // the sums start at -0: (-0) + v is v to the bit for every v, so the first frame's term is taken as it is (acc = term_0)
        float accm = -0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = make_float2(-0.f, -0.f);
        // the sums in LDS: sum q of thread i at accl[256 q], a thread's own, so no barrier orders them
        float2* accl = s + G::kFftsPerBlock * G::SF + threadIdx.x;
        if constexpr (kAccLds) {
#pragma unroll
            for (int q = 0; q < 16; ++q) accl[kFirThreads * q] = acc[q];
        }
        if (kKeepWindowCross && window) load_window<M>(window, fwd.u, w);
        if (kPrefetch) load_pairs<M>(xr, fwd.u, nx);
        for (long long t = 0; t < count; ++t) {
            // X: x's frame
            if constexpr (kPrefetch) {
#pragma unroll
                for (int q = 0; q < 16; ++q) xs[q] = nx[q];
            } else {
                load_pairs<M>(xr + t * hop, fwd.u, xs);
            }
            if (window) {
                if (!kKeepWindowCross) load_window<M>(window, per_tile(fwd.u), w);   // per_tile: loaded here, not hoisted and kept
                __builtin_amdgcn_sched_barrier(0);
                apply_window(xs, w);
            } else {
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (kPrefetch) {
                // y's frame, in flight during x's transform
                load_pairs<M>(yr + t * hop, fwd.u, r);
                __builtin_amdgcn_sched_barrier(0);
            }
            float xm, ym;
            frame_spectrum<M>(fwd, sf, xs, xm, self);
            // y's loads and the window's do not move up into the split, where Z, its partners and the twiddle row are live
            __builtin_amdgcn_sched_barrier(0);
            // Y: y's frame, through the same region (frame_spectrum starts with the fft_sync that frees it)
            if constexpr (!kPrefetch) load_pairs<M>(yr + t * hop, fwd.u, r);
            if (window) {
                if (!kKeepWindowCross) load_window<M>(window, per_tile(fwd.u), w);   // per_tile: loaded here, not hoisted and kept
                __builtin_amdgcn_sched_barrier(0);
                apply_window(r, w);
            } else {
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (kPrefetch) {
                // x's next frame, in flight during y's transform
                if (t + 1 < count) load_pairs<M>(xr + (t + 1) * hop, fwd.u, nx);
                __builtin_amdgcn_sched_barrier(0);
            }
            frame_spectrum<M>(fwd, sf, r, ym, self);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float re = xs[q].x * r[q].x + xs[q].y * r[q].y;
                const float a = xs[q].x * r[q].y;
                const float b = xs[q].y * r[q].x;
                const float im = a - b;
                if constexpr (kAccLds) {
                    const float2 old = accl[kFirThreads * q];
                    const float sre = old.x + re;
                    const float sim = old.y + im;
                    accl[kFirThreads * q] = make_float2(sre, sim);
                } else {
                    const float sre = acc[q].x + re;
                    const float sim = acc[q].y + im;
                    acc[q] = make_float2(sre, sim);
                }
            }
            const float pm = xm * ym;          // + 0 * 0
            accm = accm + pm;
        }
        if constexpr (kAccLds) {
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[q] = accl[kFirThreads * q];
        }
        // bin 0 is real in X and in Y: its imaginary part is +0, whatever sign the sum of its zero products took
        acc[0].y = self ? 0.f : acc[0].y;
        float2* orow = out + g * (M + 1);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            if (active) gstorec(orow + (fwd.u + T * q), acc[q].x, acc[q].y);
        }
        if (active && self) gstorec(orow + M, accm, 0.f);
    }
}

template <>
int launch_welch<SMFFT_WELCH_N>(const float* in, float* out, const float* window, long long total, long long groups, long long count, long long hop,
                                long long stream_stride, int grid, hipStream_t stream) {
    hipLaunchKernelGGL(welch_kernel<SMFFT_WELCH_N>, dim3((unsigned)grid), dim3(kFirThreads), 0, stream, in, out, window, total, groups, count, hop,
                       stream_stride);
    return (int)hipGetLastError();
}

template <>
int launch_csd<SMFFT_WELCH_N>(const float* x, const float* y, float2* out, const float* window, long long total, long long groups, long long count,
                              long long hop, long long x_stride, long long y_stride, int grid, hipStream_t stream) {
    hipLaunchKernelGGL(csd_kernel<SMFFT_WELCH_N>, dim3((unsigned)grid), dim3(kFirThreads), 0, stream, x, y, out, window, total, groups, count, hop,
                       x_stride, y_stride);
    return (int)hipGetLastError();
}

}  // namespace welch
}  // namespace smfft

#else  // the C ABI
#include "smfft_rows_host.hpp"

namespace {
constexpr unsigned long long kMaxElements = 1ull << 59;      // floats of a buffer: keeps the byte counts below inside 64 bits

auto dispatch_welch(const void* in, void* out, const void* window, int n, long long streams, long long groups, long long T, long long hop,
                    long long stream_stride) {
    return [=](int grid, hipStream_t stream) {
        const int M = half_length_fft_size(n);
        const long long total = streams * groups;
        grid = default_grid(M, total, grid);
        return dispatch_m(M, [&](auto m) {
            return smfft::welch::launch_welch<m()>((const float*)in, (float*)out, (const float*)window, total, groups, T, hop, stream_stride, grid, stream);
        });
    };
}

auto dispatch_csd(const void* x, const void* y, void* out, const void* window, int n, long long streams, long long groups, long long T, long long hop,
                  long long x_stride, long long y_stride) {
    return [=](int grid, hipStream_t stream) {
        const int M = half_length_fft_size(n);
        const long long total = streams * groups;
        grid = default_grid(M, total, grid);
        return dispatch_m(M, [&](auto m) {
            return smfft::welch::launch_csd<m()>((const float*)x, (const float*)y, (float2*)out, (const float*)window, total, groups, T, hop, x_stride,
                                                 y_stride, grid, stream);
        });
    };
}

// -1: refused; 0: launch; 1: nothing to do.  No HIP call.  y = nullptr: the auto spectra (floats out); else the cross spectra (complex
// out).  The output overlaps neither the range of x's frames, nor that of y's, nor the window
int check(const void* x, const void* y, const void* out, const void* window, int n, long long streams, long long groups, long long T, long long hop,
          long long x_stride, long long y_stride, bool cross) {
    const int M = half_length_fft_size(n);
    if (M < 0 || T < 1 || streams < 0 || groups < 0 || hop < 1 || x_stride < 1 || y_stride < 0) return -1;
    if (streams == 0 || groups == 0) return 1;
    // the 2^59 rule of smfft_stft.hip's check, in 128 bits: the frames of a stream first, so that no product below leaves them
    const unsigned __int128 frames = (unsigned __int128)groups * (unsigned __int128)T;
    if (frames > kMaxElements) return -1;
    const unsigned __int128 total = (unsigned __int128)streams * frames;
    const unsigned __int128 within = (frames - 1) * (unsigned __int128)hop + (unsigned)n;
    const unsigned __int128 x_extent = (unsigned __int128)(streams - 1) * (unsigned __int128)x_stride + within;
    const unsigned __int128 y_extent = (unsigned __int128)(streams - 1) * (unsigned __int128)y_stride + within;
    if (total > kMaxElements / (unsigned)n || x_extent > kMaxElements || y_extent > kMaxElements) return -1;
    // floats of the output: M + 1 powers or M + 1 complex values per group
    const unsigned long long outs = (unsigned long long)streams * (unsigned long long)groups * (unsigned)(M + 1) * (cross ? 2u : 1u);
    if (overlap(x, (unsigned long long)x_extent, out, outs)) return -1;
    if (cross && overlap(y, (unsigned long long)y_extent, out, outs)) return -1;
    if (window && overlap(window, (unsigned)n, out, outs)) return -1;
    return 0;
}

int check_welch(const void* in, const void* out, const void* window, int n, long long streams, long long groups, long long T, long long hop,
                long long stream_stride) {
    return check(in, nullptr, out, window, n, streams, groups, T, hop, stream_stride, 0, false);
}
}  // namespace

extern "C" {

int smfft_welch_fft_size(int n) { return half_length_fft_size(n); }

long long smfft_welch_groups(long long L, int n, long long hop, long long T) {
    if (half_length_fft_size(n) < 0 || hop < 1 || T < 1 || L < 0) return -1;
    return L < n ? 0 : (1 + (L - n) / hop) / T;
}

int smfft_welch_launch(const void* d_in, void* d_out, const void* d_window, int n, long long streams, long long groups, long long T, long long hop, long long stream_stride, void* hip_stream) {
    return checked_launch(check_welch(d_in, d_out, d_window, n, streams, groups, T, hop, stream_stride),
                          dispatch_welch(d_in, d_out, d_window, n, streams, groups, T, hop, stream_stride), hip_stream);
}

int smfft_welch_launch_tuned(const void* d_in, void* d_out, const void* d_window, int n, long long streams, long long groups, long long T, long long hop, long long stream_stride, void* hip_stream, int grid) {
    return checked_launch_tuned(check_welch(d_in, d_out, d_window, n, streams, groups, T, hop, stream_stride),
                                dispatch_welch(d_in, d_out, d_window, n, streams, groups, T, hop, stream_stride), hip_stream, grid);
}

int smfft_welch_benchmark(const void* d_in, void* d_out, const void* d_window, int n, long long streams, long long groups, long long T, long long hop, long long stream_stride, double* FFT_time) {
    return checked_benchmark(check_welch(d_in, d_out, d_window, n, streams, groups, T, hop, stream_stride),
                             dispatch_welch(d_in, d_out, d_window, n, streams, groups, T, hop, stream_stride), FFT_time);
}

int smfft_csd_launch(const void* d_x, const void* d_y, void* d_out, const void* d_window, int n, long long streams, long long groups, long long T, long long hop, long long x_stride, long long y_stride, void* hip_stream) {
    return checked_launch(check(d_x, d_y, d_out, d_window, n, streams, groups, T, hop, x_stride, y_stride, true),
                          dispatch_csd(d_x, d_y, d_out, d_window, n, streams, groups, T, hop, x_stride, y_stride), hip_stream);
}

int smfft_csd_launch_tuned(const void* d_x, const void* d_y, void* d_out, const void* d_window, int n, long long streams, long long groups, long long T, long long hop, long long x_stride, long long y_stride, void* hip_stream, int grid) {
    return checked_launch_tuned(check(d_x, d_y, d_out, d_window, n, streams, groups, T, hop, x_stride, y_stride, true),
                                dispatch_csd(d_x, d_y, d_out, d_window, n, streams, groups, T, hop, x_stride, y_stride), hip_stream, grid);
}

int smfft_csd_benchmark(const void* d_x, const void* d_y, void* d_out, const void* d_window, int n, long long streams, long long groups, long long T, long long hop, long long x_stride, long long y_stride, double* FFT_time) {
    return checked_benchmark(check(d_x, d_y, d_out, d_window, n, streams, groups, T, hop, x_stride, y_stride, true),
                             dispatch_csd(d_x, d_y, d_out, d_window, n, streams, groups, T, hop, x_stride, y_stride), FFT_time);
}

}  // extern "C"
#endif

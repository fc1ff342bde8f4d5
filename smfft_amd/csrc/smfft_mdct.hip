// smfft_mdct.hip -- libsmfft_mdct.so: batched DCT-IV / DST-IV of real rows of n = 512 ... 8192 points (powers of two) and the MDCT / IMDCT
// of N = 512 ... 8192 coefficients per frame of 2 N samples, un-normalised, on ONE complex transform of M = n / 2 = 256 ... 4096 points of
// the register engine per row or frame, in one kernel and one pass through HBM, and the C ABI of include/smfft_mdct.h.
//
// Compiled once per M (Makefile: -DSMFFT_MDCT_N=256 ... 4096, flags of their own: MDCT_FLAGS_<M>) for the three kernels and their
// launchers, and once without SMFFT_MDCT_N for the C ABI, which checks and dispatches.
//
// The kernels keep the geometry of dct2_kernel<M> (smfft_dct.hip: 256 threads, 4096 / M rows per workgroup, element u + T q in register
// q, workgroups stride over the tiles).  With p, k < M:
//     t[p] = (x[2p] + i x[n-1-2p]) exp(-i pi (4p+1) / (4n));  T = DFT_M(t);  Y[k] = T[k] exp(-i pi k / n);
//     X[2k] = 2 Re Y[k];  X[n-1-2k] = -2 Im Y[k]
// is the DCT-IV: one twiddle in front of the transform and one behind it, no Hermitian split and no partner exchange, and the same
// index map on both sides -- with E[j] = x[2j] and O[j] = x[2j+1] the even and the odd samples of a row, element p takes E[p] and
// O[M-1-p], and gives them.
// dct4_kernel: that, and the sine transform as a runtime argument: DST-IV(x)[k] = (-1)^k DCT-IV(reverse x)[k], which swaps the two
//     samples of an element on the load side and drops the minus of the odd outputs on the store side.
// mdct_kernel: X = DCT-IV_N(u) / 2 with u = [-c_r - d, a - b_r] the fold of the windowed frame v = w x = [a, b, c, d] (quarters of
//     N / 2 = M samples, _r reversed).  The half [a, b] gives the imaginary parts of the elements p < M / 2 and the real parts of the
//     others, the half [c, d] the rest: the frame is folded in two halves of n floats, each through the row's LDS region.
// imdct_kernel: y = w [D[M:], -reverse(D), -D[:M]] with D = DCT-IV_N(X) / 2: every D goes to two of the 2 N outputs.
//
// How a row reaches the registers and leaves them: 16-byte accesses x[4c ... 4c+3] (4-byte aligned: the rows' contract), which hold
// E[2c], O[2c], E[2c+1], O[2c+1].  They pass through the row's LDS region, E at floats [0, M) and O at [M, 2 M) -- a row of n floats
// fills the M float2 of the region exactly -- where element p reads or writes E[p] and O[M-1-p], consecutive floats per lane on both
// sides.  -DSMFFT_MDCT_STAGED=0 builds 4-byte accesses at a stride of two floats per lane instead, with no pass through LDS
// (MDCT_STAGED=0 in the Makefile builds it beside the shipped library; tools/ab_mdct.py times it).
//
// Twiddles: exp(-i pi k / n) = W_32768^{k 16384 / n} and exp(-i pi (4p+1) / (4n)) = W_65536^{(4p+1) 8192 / n} are rows built at compile
// time, one entry per element so that the lanes of a row read consecutive addresses, from the fp64-rounded first octant of W_32768
// (smfft_twiddles_dct.inc through smfft_rows.hpp) and, for the odd indices that n = 8192 needs, from the odd entries of the first octant of W_65536
// (smfft_twiddles_mdct.inc, tools/gen_twiddles_mdct.py), extended by exact symmetries.  No v_sin / v_cos.
//
// In place (dct4, d_out == d_in) is served: every value a workgroup loads from a row is in LDS or in registers in front of the first
// exchange behind the loads, and the stores come behind the transform; rows belong to one workgroup.
//
// Cache policy: the 16-byte row accesses carry the engine's policy (non-temporal; -DSMFFT_NT=0 builds them plain,
// -DSMFFT_MDCT_NT_LOAD4 / -DSMFFT_MDCT_NT_STORE4 one of them), the 4-byte ones of the other build are plain (-DSMFFT_MDCT_NT_LOAD1=1 /
// -DSMFFT_MDCT_NT_STORE1=1 build them non-temporal), the window is always loaded plain: every frame reads it.
//
// -ffp-contract=on (Makefile, MDCT_FLAGS_<M>): a product is fused into a sum only where one expression of the source writes both, so
// every build of this file rounds alike and the A/B builds give the shipped build's bits.  The windowed samples are products of
// their own statement, for that reason.
#include <hip/hip_runtime.h>

#include "smfft_mdct.h"

namespace smfft {
namespace mdct {
// enqueue `grid` workgroups on `stream`; 0 or the launch's hipError_t.  Defined per M by the objects compiled with -DSMFFT_MDCT_N.
template <int M>
int launch_dct4(const float* in, float* out, long long batch, int sine, int grid, hipStream_t stream);
template <int M>
int launch_mdct(const float* in, float* out, const float* window, long long total, long long frames, long long hop, long long stream_stride, int grid,
                hipStream_t stream);
template <int M>
int launch_imdct(const float* in, float* out, const float* window, long long batch, int grid, hipStream_t stream);
}  // namespace mdct
}  // namespace smfft

#ifdef SMFFT_MDCT_N
#include "smfft_fir_kernel.hpp"
#include "smfft_rows.hpp"

// 1: 16-byte row accesses and a pass through the row's LDS region; 0: 4-byte row accesses at stride two
#ifndef SMFFT_MDCT_STAGED
#define SMFFT_MDCT_STAGED 1
#endif

// the policy of the 16-byte and of the 4-byte row loads and stores: 1 non-temporal, 0 plain
#ifndef SMFFT_MDCT_NT_LOAD4
#define SMFFT_MDCT_NT_LOAD4 SMFFT_NT
#endif
#ifndef SMFFT_MDCT_NT_STORE4
#define SMFFT_MDCT_NT_STORE4 SMFFT_NT
#endif
#ifndef SMFFT_MDCT_NT_LOAD1
#define SMFFT_MDCT_NT_LOAD1 0
#endif
#ifndef SMFFT_MDCT_NT_STORE1
#define SMFFT_MDCT_NT_STORE1 0
#endif

namespace smfft {
namespace mdct {

using rows::w32768, rows::row_entry, rows::per_tile, rows::row_quad;

static constexpr TwiddleValue odd_octant_65536[4096] = {
#include "smfft/smfft_twiddles_mdct.inc"
};

// (cos, sin)(2 pi m / 65536), 0 <= m < 16384: the even m are entries of W_32768, the odd ones below pi / 4 are the table's, and
// (cos, sin)(pi / 2 - t) = (sin, cos)(t) takes the odd ones beyond it to those
constexpr TwiddleValue w65536(int m) {
    if (m % 2 == 0) return w32768(m / 2);
    if (m < 8192) return odd_octant_65536[(m - 1) / 2];
    const TwiddleValue b = odd_octant_65536[(16384 - m - 1) / 2];
    return TwiddleValue{b.y, b.x};
}

// the twiddle rows of n = 2 M points as (cos, sin), that is the CONJUGATES of exp(-i pi (4p+1) / (4n)) and exp(-i pi k / n)
template <int M>
struct Rows {
    TwiddleValue pre[M];         // angle pi (4p+1) / (4n) = 2 pi (4p+1) (4096 / M) / 65536
    TwiddleValue post[M];        // angle pi k / n = 2 pi k (8192 / M) / 32768
    constexpr Rows() : pre{}, post{} {
        for (int p = 0; p < M; ++p) pre[p] = w65536((4 * p + 1) * (4096 / M));
        for (int k = 0; k < M; ++k) post[k] = w32768(k * (8192 / M));
    }
};
template <int M>
static __device__ const Rows<M> rows = Rows<M>();

// one float, or four consecutive floats at 4-byte alignment, with the policies above
__device__ __forceinline__ float gload1(const float* p) { return rows::gload1<SMFFT_MDCT_NT_LOAD1 != 0>(p); }
__device__ __forceinline__ void gstore1(float* p, float v) { rows::gstore1<SMFFT_MDCT_NT_STORE1 != 0>(p, v); }
__device__ __forceinline__ row_quad gload4(const float* p) { return rows::gload4<SMFFT_MDCT_NT_LOAD4 != 0>(p); }
__device__ __forceinline__ void gstore4(float* p, row_quad v) { rows::gstore4<SMFFT_MDCT_NT_STORE4 != 0>(p, v); }
// the window: plain loads, every frame reads it
__device__ __forceinline__ row_quad wload4(const float* p) { return rows::gload4<false>(p); }

// two consecutive floats of a row's LDS region, at an even float index
__device__ __forceinline__ float2 lds_pair(const float* fl, int i) { return *reinterpret_cast<const float2*>(fl + i); }

// the quad x[4c ... 4c+3] = E[2c], O[2c], E[2c+1], O[2c+1] into the region: E at floats [0, M), O at [M, 2 M)
template <int M>
__device__ __forceinline__ void stage_quad(float* fl, int c, row_quad f) {
    *reinterpret_cast<float2*>(fl + 2 * c) = make_float2(f.x, f.z);
    *reinterpret_cast<float2*>(fl + M + 2 * c) = make_float2(f.y, f.w);
}

// r[q] = (a[q] + i b[q]) exp(-i pi (4p+1) / (4n)), p = u + T q
template <int M>
__device__ __forceinline__ void pre_twiddle(float2 (&r)[16], const float (&a)[16], const float (&b)[16], int u) {
    constexpr int T = Geometry<M>::T;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const float2 w = row_entry(&rows<M>.pre[u + T * q]);
        r[q] = make_float2(a[q] * w.x + b[q] * w.y, b[q] * w.x - a[q] * w.y);
    }
}

// o0[q] = s0 Re Y[k], o1[q] = s1 Im Y[k], Y[k] = r[q] exp(-i pi k / n), k = u + T q
template <int M>
__device__ __forceinline__ void post_twiddle(const float2 (&r)[16], float (&o0)[16], float (&o1)[16], int u, float s0, float s1) {
    constexpr int T = Geometry<M>::T;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const float2 w = row_entry(&rows<M>.post[u + T * q]);
        const float yx = r[q].x * w.x + r[q].y * w.y, yy = r[q].y * w.x - r[q].x * w.y;
        o0[q] = s0 * yx;
        o1[q] = s1 * yy;
    }
}

// out[r n + .] = DCT-IV (sine == 0) or DST-IV of in[r n + .], n = 2 M.  in and out may be the same buffer: no __restrict__.
template <int M>
__global__ void __launch_bounds__(kFirThreads) dct4_kernel(const float* in, float* out, long long batch, int sine) {
    using G = Geometry<M>;
    constexpr int T = G::T, n = 2 * M;
    __shared__ float2 s[G::kFftsPerBlock * G::SF];
    Engine<M, 0, 1> fwd;
    fwd.init(threadIdx.x);
    float2* sf = s + fwd.fft * G::SF;
    [[maybe_unused]] float* fl = reinterpret_cast<float*>(sf);     // the region as floats: E at [0, M), O at [M, 2 M)
    const long long ntiles = (batch + G::kFftsPerBlock - 1) / G::kFftsPerBlock;
    const float s1 = sine ? 2.f : -2.f;        // of the odd outputs: X[n-1-2k] = -2 Im Y[k], and (-1)^(n-1-2k) = -1 for the sine transform
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long g = tile * G::kFftsPerBlock + fwd.fft;
        const bool active = g < batch;
        // an inactive slot of the last tile reads row 0 and stores nothing
        const float* xr = in + (active ? g : 0) * n;
        float a[16], b[16];
#if SMFFT_MDCT_STAGED
        row_quad f[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) f[q] = gload4(xr + 4 * (fwd.u + T * q));
        __builtin_amdgcn_sched_barrier(0);
        fft_sync<G::kMultiWave>();             // the previous tile's store-side reads are done with the region
#pragma unroll
        for (int q = 0; q < 8; ++q) stage_quad<M>(fl, fwd.u + T * q, f[q]);
        fft_sync<G::kMultiWave>();
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int p = fwd.u + T * q;
            a[q] = fl[p];                      // x[2p]
            b[q] = fl[M + M - 1 - p];          // x[n-1-2p]
        }
#else
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int p = fwd.u + T * q;
            a[q] = gload1(xr + 2 * p);
            b[q] = gload1(xr + n - 1 - 2 * p);
        }
        // nothing is scheduled across this point: the 32 loads all go out before the first arithmetic
        __builtin_amdgcn_sched_barrier(0);
#endif
        // the sine transform reads the row reversed: the two samples of an element change places
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float x0 = a[q], x1 = b[q];
            a[q] = sine ? x1 : x0;
            b[q] = sine ? x0 : x1;
        }
        const int u = per_tile(fwd.u);
        float2 r[16];
        pre_twiddle<M>(r, a, b, u);
        fft_sync<G::kMultiWave>();             // the region is free: the staging reads above, or the previous tile
        fwd.transform(r, sf);
        post_twiddle<M>(r, a, b, u, 2.f, s1);
        float* yr = out + g * n;
#if SMFFT_MDCT_STAGED
        fft_sync<G::kMultiWave>();             // the transform's last LDS reads are done
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int k = fwd.u + T * q;
            fl[k] = a[q];                      // X[2k]
            fl[M + M - 1 - k] = b[q];          // X[n-1-2k]
        }
        fft_sync<G::kMultiWave>();
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int c = fwd.u + T * q;
            const float2 e = lds_pair(fl, 2 * c), o = lds_pair(fl, M + 2 * c);
            const row_quad f4 = {e.x, o.x, e.y, o.y};
            if (active) gstore4(yr + 4 * c, f4);
        }
#else
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int k = fwd.u + T * q;
            if (active) {
                gstore1(yr + 2 * k, a[q]);
                gstore1(yr + n - 1 - 2 * k, b[q]);
            }
        }
#endif
    }
}

// out[g N + .] = MDCT of the frame in[c stream_stride + f hop + .] of 2 N samples, g = c frames + f < total, N = 2 M, under
// window[0, 2 N) (null: all ones)
template <int M>
__global__ void __launch_bounds__(kFirThreads) mdct_kernel(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ window,
                                                           long long total, long long frames, long long hop, long long stream_stride) {
    using G = Geometry<M>;
    constexpr int T = G::T, N = 2 * M;
    __shared__ float2 s[G::kFftsPerBlock * G::SF];
    Engine<M, 0, 1> fwd;
    fwd.init(threadIdx.x);
    float2* sf = s + fwd.fft * G::SF;
    [[maybe_unused]] float* fl = reinterpret_cast<float*>(sf);     // the region as floats: E at [0, M), O at [M, 2 M)
    const long long ntiles = (total + G::kFftsPerBlock - 1) / G::kFftsPerBlock;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long g = tile * G::kFftsPerBlock + fwd.fft;
        const bool active = g < total;
        // an inactive slot of the last tile reads frame 0 and stores nothing
        const long long gg = active ? g : 0;
        const long long c = gg / frames;
        const float* xr = in + c * stream_stride + (gg - c * frames) * hop;
        float a[16], b[16];
#if SMFFT_MDCT_STAGED
        // the frame in two halves of N floats, [a, b] and [c, d]: eight 16-byte loads of samples and eight of the window each, the
        // products through the region as a row's are
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            row_quad f[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) f[q] = gload4(xr + h * N + 4 * (fwd.u + T * q));
            if (window) {
                row_quad w[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) w[q] = wload4(window + h * N + 4 * (fwd.u + T * q));
#pragma unroll
                for (int q = 0; q < 8; ++q) f[q] = f[q] * w[q];
            }
            fft_sync<G::kMultiWave>();         // the first half's reads, or the previous tile's store-side reads, are done
#pragma unroll
            for (int q = 0; q < 8; ++q) stage_quad<M>(fl, fwd.u + T * q, f[q]);
            fft_sync<G::kMultiWave>();
            // E[j] = v[h N + 2j], O[j] = v[h N + 2j + 1], j < M
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int p = fwd.u + T * q;
                if (h == 0) {
                    if (q < 8) b[q] = fl[M + M / 2 - 1 - p] - fl[M / 2 + p];                  // v[M-1-2p] - v[M+2p]
                    else a[q] = fl[p - M / 2] - fl[M + M + M / 2 - 1 - p];                   // v[2p-M] - v[N+M-1-2p]
                } else {
                    if (q < 8) a[q] = -fl[M + M / 2 - 1 - p] - fl[M / 2 + p];                 // -v[N+M-1-2p] - v[N+M+2p]
                    else b[q] = -fl[p - M / 2] - fl[M + M + M / 2 - 1 - p];                  // -v[M+2p] - v[2N+M-1-2p]
                }
            }
        }
#else
        float x0[16], x1[16], x2[16], x3[16];
        // element p: Re from v[i0], v[i1], Im from v[i2], v[i3]
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int p = fwd.u + T * q;
            const int i0 = q < 8 ? N + M - 1 - 2 * p : 2 * p - M, i1 = q < 8 ? N + M + 2 * p : N + M - 1 - 2 * p;
            const int i2 = q < 8 ? M - 1 - 2 * p : M + 2 * p, i3 = q < 8 ? M + 2 * p : 2 * N + M - 1 - 2 * p;
            x0[q] = gload1(xr + i0);
            x1[q] = gload1(xr + i1);
            x2[q] = gload1(xr + i2);
            x3[q] = gload1(xr + i3);
        }
        if (window) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int p = fwd.u + T * q;
                const int i0 = q < 8 ? N + M - 1 - 2 * p : 2 * p - M, i1 = q < 8 ? N + M + 2 * p : N + M - 1 - 2 * p;
                const int i2 = q < 8 ? M - 1 - 2 * p : M + 2 * p, i3 = q < 8 ? M + 2 * p : 2 * N + M - 1 - 2 * p;
                const float w0 = window[i0], w1 = window[i1], w2 = window[i2], w3 = window[i3];
                x0[q] = x0[q] * w0;
                x1[q] = x1[q] * w1;
                x2[q] = x2[q] * w2;
                x3[q] = x3[q] * w3;
            }
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            a[q] = q < 8 ? -x0[q] - x1[q] : x0[q] - x1[q];
            b[q] = q < 8 ? x2[q] - x3[q] : -x2[q] - x3[q];
        }
#endif
        const int u = per_tile(fwd.u);
        float2 r[16];
        pre_twiddle<M>(r, a, b, u);
        fft_sync<G::kMultiWave>();             // the region is free: the fold's reads above, or the previous tile
        fwd.transform(r, sf);
        post_twiddle<M>(r, a, b, u, 1.f, -1.f);
        float* yr = out + g * N;
#if SMFFT_MDCT_STAGED
        fft_sync<G::kMultiWave>();             // the transform's last LDS reads are done
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int k = fwd.u + T * q;
            fl[k] = a[q];                      // X[2k]
            fl[M + M - 1 - k] = b[q];          // X[N-1-2k]
        }
        fft_sync<G::kMultiWave>();
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int cq = fwd.u + T * q;
            const float2 e = lds_pair(fl, 2 * cq), o = lds_pair(fl, M + 2 * cq);
            const row_quad f4 = {e.x, o.x, e.y, o.y};
            if (active) gstore4(yr + 4 * cq, f4);
        }
#else
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int k = fwd.u + T * q;
            if (active) {
                gstore1(yr + 2 * k, a[q]);
                gstore1(yr + N - 1 - 2 * k, b[q]);
            }
        }
#endif
    }
}

// out[r 2 N + .] = IMDCT of in[r N + .], N = 2 M, under window[0, 2 N) (null: all ones)
template <int M>
__global__ void __launch_bounds__(kFirThreads) imdct_kernel(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ window,
                                                            long long batch) {
    using G = Geometry<M>;
    constexpr int T = G::T, N = 2 * M;
    __shared__ float2 s[G::kFftsPerBlock * G::SF];
    Engine<M, 0, 1> fwd;
    fwd.init(threadIdx.x);
    float2* sf = s + fwd.fft * G::SF;
    [[maybe_unused]] float* fl = reinterpret_cast<float*>(sf);     // the region as floats: E at [0, M), O at [M, 2 M)
    const long long ntiles = (batch + G::kFftsPerBlock - 1) / G::kFftsPerBlock;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long g = tile * G::kFftsPerBlock + fwd.fft;
        const bool active = g < batch;
        const float* xr = in + (active ? g : 0) * N;
        float a[16], b[16];
#if SMFFT_MDCT_STAGED
        row_quad f[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) f[q] = gload4(xr + 4 * (fwd.u + T * q));
        __builtin_amdgcn_sched_barrier(0);
        fft_sync<G::kMultiWave>();             // the previous tile's store-side reads are done with the region
#pragma unroll
        for (int q = 0; q < 8; ++q) stage_quad<M>(fl, fwd.u + T * q, f[q]);
        fft_sync<G::kMultiWave>();
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int p = fwd.u + T * q;
            a[q] = fl[p];
            b[q] = fl[M + M - 1 - p];
        }
#else
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int p = fwd.u + T * q;
            a[q] = gload1(xr + 2 * p);
            b[q] = gload1(xr + N - 1 - 2 * p);
        }
        __builtin_amdgcn_sched_barrier(0);
#endif
        const int u = per_tile(fwd.u);
        float2 r[16];
        pre_twiddle<M>(r, a, b, u);
        fft_sync<G::kMultiWave>();
        fwd.transform(r, sf);
        post_twiddle<M>(r, a, b, u, 1.f, -1.f);          // a[q] = D[2k], b[q] = D[N-1-2k]
        float* yr = out + g * (2 * N);
#if SMFFT_MDCT_STAGED
        fft_sync<G::kMultiWave>();             // the transform's last LDS reads are done
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int k = fwd.u + T * q;
            fl[k] = a[q];                      // E[k] = D[2k]
            fl[M + M - 1 - k] = b[q];          // O[M-1-k] = D[N-1-2k]
        }
        fft_sync<G::kMultiWave>();
        // the 2 N outputs as sixteen quads per thread: y[4c ... 4c+3], c = u + T q
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int c = fwd.u + T * q;
            row_quad y;
            if (q < 4) {                       // y[j] = D[M + j]
                const float2 e = lds_pair(fl, M / 2 + 2 * c), o = lds_pair(fl, M + M / 2 + 2 * c);
                y = row_quad{e.x, o.x, e.y, o.y};
            } else if (q < 12) {               // y[j] = -D[3 M - 1 - j]
                const int i = 3 * M / 2 - 2 - 2 * c;
                const float2 o = lds_pair(fl, M + i), e = lds_pair(fl, i);
                y = row_quad{-o.y, -e.y, -o.x, -e.x};
            } else {                           // y[j] = -D[j - 3 M]
                const int i = 2 * c - 3 * M / 2;
                const float2 e = lds_pair(fl, i), o = lds_pair(fl, M + i);
                y = row_quad{-e.x, -o.x, -e.y, -o.y};
            }
            if (window) {
                const row_quad w = wload4(window + 4 * c);
                y = y * w;
            }
            if (active) gstore4(yr + 4 * c, y);
        }
#else
        // D[m], m >= M, goes to y[m - M] and, negated, to y[3 M - 1 - m]; m < M, negated, to y[3 M - 1 - m] and y[3 M + m]
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int k = fwd.u + T * q;
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                const int m = side == 0 ? 2 * k : N - 1 - 2 * k;
                const bool upper = side == 0 ? q >= 8 : q < 8;       // m >= M
                const float d = side == 0 ? a[q] : b[q];
                const int j0 = upper ? m - M : 3 * M + m, j1 = 3 * M - 1 - m;
                float y0 = upper ? d : -d, y1 = -d;
                if (window) {
                    const float w0 = window[j0], w1 = window[j1];
                    y0 = y0 * w0;
                    y1 = y1 * w1;
                }
                if (active) {
                    gstore1(yr + j0, y0);
                    gstore1(yr + j1, y1);
                }
            }
        }
#endif
    }
}

template <>
int launch_dct4<SMFFT_MDCT_N>(const float* in, float* out, long long batch, int sine, int grid, hipStream_t stream) {
    hipLaunchKernelGGL(dct4_kernel<SMFFT_MDCT_N>, dim3((unsigned)grid), dim3(kFirThreads), 0, stream, in, out, batch, sine);
    return (int)hipGetLastError();
}

template <>
int launch_mdct<SMFFT_MDCT_N>(const float* in, float* out, const float* window, long long total, long long frames, long long hop,
                              long long stream_stride, int grid, hipStream_t stream) {
    hipLaunchKernelGGL(mdct_kernel<SMFFT_MDCT_N>, dim3((unsigned)grid), dim3(kFirThreads), 0, stream, in, out, window, total, frames, hop, stream_stride);
    return (int)hipGetLastError();
}

template <>
int launch_imdct<SMFFT_MDCT_N>(const float* in, float* out, const float* window, long long batch, int grid, hipStream_t stream) {
    hipLaunchKernelGGL(imdct_kernel<SMFFT_MDCT_N>, dim3((unsigned)grid), dim3(kFirThreads), 0, stream, in, out, window, batch);
    return (int)hipGetLastError();
}

}  // namespace mdct
}  // namespace smfft

#else  // the C ABI
#include "smfft_rows_host.hpp"

namespace {
constexpr unsigned long long kMaxElements = 1ull << 60;      // of a buffer: keeps the byte counts below inside 64 bits

// the launches of `grid` workgroups (<= 0: the default) on `stream`
auto dispatch_dct4(const void* in, void* out, int n, long long batch, int sine) {
    return [=](int grid, hipStream_t stream) {
        const int M = half_length_fft_size(n);
        grid = default_grid(M, batch, grid);
        return dispatch_m(M, [&](auto m) { return smfft::mdct::launch_dct4<m()>((const float*)in, (float*)out, batch, sine != 0, grid, stream); });
    };
}

auto dispatch_mdct(const void* in, void* out, const void* window, int N, long long streams, long long frames, long long hop, long long stream_stride) {
    return [=](int grid, hipStream_t stream) {
        const int M = half_length_fft_size(N);
        const long long total = streams * frames;
        grid = default_grid(M, total, grid);
        return dispatch_m(M, [&](auto m) {
            return smfft::mdct::launch_mdct<m()>((const float*)in, (float*)out, (const float*)window, total, frames, hop, stream_stride, grid, stream);
        });
    };
}

auto dispatch_imdct(const void* in, void* out, const void* window, int N, long long batch) {
    return [=](int grid, hipStream_t stream) {
        const int M = half_length_fft_size(N);
        grid = default_grid(M, batch, grid);
        return dispatch_m(M, [&](auto m) { return smfft::mdct::launch_imdct<m()>((const float*)in, (float*)out, (const float*)window, batch, grid, stream); });
    };
}

// -1: refused; 0: launch; 1: nothing to do.  No HIP call.
// dct4: the output is the input (in place) or does not overlap it
int check_dct4(const void* in, const void* out, int n, long long batch) {
    if (half_length_fft_size(n) < 0 || batch < 0) return -1;
    if (batch == 0) return 1;
    if ((unsigned long long)batch > kMaxElements / (unsigned)n) return -1;
    const unsigned long long count = (unsigned long long)batch * (unsigned)n;
    if (in != out && overlap(in, count, out, count)) return -1;
    return 0;
}

// mdct: the output overlaps neither the range of the frames nor the window
int check_mdct(const void* in, const void* out, const void* window, int N, long long streams, long long frames, long long hop, long long stream_stride) {
    if (half_length_fft_size(N) < 0 || streams < 0 || frames < 0 || hop < 1 || stream_stride < 1) return -1;
    if (streams == 0 || frames == 0) return 1;
    const unsigned __int128 total = (unsigned __int128)streams * (unsigned __int128)frames;
    const unsigned __int128 extent = (unsigned __int128)(streams - 1) * (unsigned __int128)stream_stride
                                     + (unsigned __int128)(frames - 1) * (unsigned __int128)hop + 2u * (unsigned)N;
    if (total > kMaxElements / (unsigned)N || extent > kMaxElements) return -1;
    const unsigned long long outs = (unsigned long long)total * (unsigned)N;
    if (overlap(in, (unsigned long long)extent, out, outs)) return -1;
    if (window && overlap(window, 2ull * (unsigned)N, out, outs)) return -1;
    return 0;
}

// imdct: the output overlaps neither the input nor the window
int check_imdct(const void* in, const void* out, const void* window, int N, long long batch) {
    if (half_length_fft_size(N) < 0 || batch < 0) return -1;
    if (batch == 0) return 1;
    if ((unsigned long long)batch > kMaxElements / (2u * (unsigned)N)) return -1;
    const unsigned long long ins = (unsigned long long)batch * (unsigned)N;
    if (overlap(in, ins, out, 2 * ins)) return -1;
    if (window && overlap(window, 2ull * (unsigned)N, out, 2 * ins)) return -1;
    return 0;
}
}  // namespace

extern "C" {

int smfft_mdct_fft_size(int n) { return half_length_fft_size(n); }

int smfft_dct4_launch(const void* d_in, void* d_out, int n, long long batch, int sine, void* hip_stream) {
    return checked_launch(check_dct4(d_in, d_out, n, batch), dispatch_dct4(d_in, d_out, n, batch, sine), hip_stream);
}

int smfft_dct4_launch_tuned(const void* d_in, void* d_out, int n, long long batch, int sine, void* hip_stream, int grid) {
    return checked_launch_tuned(check_dct4(d_in, d_out, n, batch), dispatch_dct4(d_in, d_out, n, batch, sine), hip_stream, grid);
}

int smfft_dct4_benchmark(const void* d_in, void* d_out, int n, long long batch, int sine, double* FFT_time) {
    return checked_benchmark(check_dct4(d_in, d_out, n, batch), dispatch_dct4(d_in, d_out, n, batch, sine), FFT_time);
}

int smfft_mdct_launch(const void* d_in, void* d_out, const void* d_window, int N, long long streams, long long frames, long long hop, long long stream_stride, void* hip_stream) {
    return checked_launch(check_mdct(d_in, d_out, d_window, N, streams, frames, hop, stream_stride),
                          dispatch_mdct(d_in, d_out, d_window, N, streams, frames, hop, stream_stride), hip_stream);
}

int smfft_mdct_launch_tuned(const void* d_in, void* d_out, const void* d_window, int N, long long streams, long long frames, long long hop, long long stream_stride, void* hip_stream, int grid) {
    return checked_launch_tuned(check_mdct(d_in, d_out, d_window, N, streams, frames, hop, stream_stride),
                                dispatch_mdct(d_in, d_out, d_window, N, streams, frames, hop, stream_stride), hip_stream, grid);
}

int smfft_mdct_benchmark(const void* d_in, void* d_out, const void* d_window, int N, long long streams, long long frames, long long hop, long long stream_stride, double* FFT_time) {
    return checked_benchmark(check_mdct(d_in, d_out, d_window, N, streams, frames, hop, stream_stride),
                             dispatch_mdct(d_in, d_out, d_window, N, streams, frames, hop, stream_stride), FFT_time);
}

int smfft_imdct_launch(const void* d_in, void* d_out, const void* d_window, int N, long long batch, void* hip_stream) {
    return checked_launch(check_imdct(d_in, d_out, d_window, N, batch), dispatch_imdct(d_in, d_out, d_window, N, batch), hip_stream);
}

int smfft_imdct_launch_tuned(const void* d_in, void* d_out, const void* d_window, int N, long long batch, void* hip_stream, int grid) {
    return checked_launch_tuned(check_imdct(d_in, d_out, d_window, N, batch), dispatch_imdct(d_in, d_out, d_window, N, batch), hip_stream, grid);
}

int smfft_imdct_benchmark(const void* d_in, void* d_out, const void* d_window, int N, long long batch, double* FFT_time) {
    return checked_benchmark(check_imdct(d_in, d_out, d_window, N, batch), dispatch_imdct(d_in, d_out, d_window, N, batch), FFT_time);
}

}  // extern "C"
#endif

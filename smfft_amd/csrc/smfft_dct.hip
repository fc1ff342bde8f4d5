// smfft_dct.hip -- libsmfft_dct.so: batched DCT-II / DCT-III / DST-II / DST-III of real rows of n = 512 ... 8192 points (powers of two),
// un-normalised, on ONE complex transform of M = n / 2 = 256 ... 4096 points of the register engine per row, in one kernel and one pass
// through HBM (n floats in, n floats out), and the C ABI of include/smfft_dct.h.
//
// Compiled once per M (Makefile: -DSMFFT_DCT_N=256 ... 4096, flags of their own: DCT_FLAGS_<M>) for the two kernels and their launcher,
// and once without SMFFT_DCT_N for the C ABI, which checks and dispatches.
//
// Both kernels keep the geometry of rowconv_real_kernel<M> (smfft_rowconv_real.hip: 256 threads, 4096 / M rows per workgroup, element
// u + T q in register q, workgroups stride over the tiles).  With v the permuted row, v[j] = x[2j], v[n - 1 - j] = x[2j + 1], the even
// and the odd samples of v are the two lanes of the transform, z[p] = v[2p] + i v[2p + 1]:
//     p <  M / 2:  z[p] = x[4p]         + i x[4p + 2]
//     p >= M / 2:  z[p] = x[2n - 1 - 4p] + i x[2n - 3 - 4p]
// dct2_kernel: Z = DFT_M(z); partner P[k] = conj Z[(M - k) mod M] through the row's LDS region (the form of rowconv_real_kernel);
//     S = Z + P, D = Z - P, V = S - i W_n^k D (twice the n-point spectrum of v), Y = W_4n^k V; X[k] = Re Y[k], X[n - k] = -Im Y[k],
//     and X[M] = 2 cos(pi / 4) (Re Z[0] - Im Z[0]) from the thread that holds k = 0.  The stores are consecutive floats per lane.
// dct3_kernel: V'[k] = conj(W_4n^k) (X[k] - i X[n - k]) (X[n] := 0) from consecutive floats per lane; the partner V'[M - k] through the
//     row's LDS region as well (V'[M], which no thread owns, from the thread of k = 0: read straight from global memory instead, the
//     sixty-four loads and forty-eight twiddles of a thread need 258 ... 277 VGPRs at M = 1024 / 2048);
//     Z[k] = (V'[k] + conj V'[M - k]) + i conj(W_n^k) (V'[k] - conj V'[M - k]); z = the un-normalised inverse transform; y[.] = the index
//     map above, backwards.  DCT-III(DCT-II(x)) = 2n x.
// The sine transforms are runtime arguments of the same kernels: DST-II(x)[k] = DCT-II(s x)[n - 1 - k] and
// DST-III(X)[j] = s_j DCT-III(reverse X)[j] with s_j = (-1)^j -- a minus on the second half of z and the other side's index reversed.
//
// How the permuted row reaches the registers (and, type III, leaves them): eight 16-byte accesses x[4p ... 4p + 3], p < M / 2, per thread
// (4-byte aligned: the rows' contract), which hold z[p] and, as (x[4p + 3], x[4p + 1]), z[M - 1 - p]: that half goes through the row's
// LDS region to (or comes from) the thread that owns it.  -DSMFFT_DCT_STAGED=0 builds sixteen pairs of 4-byte accesses at a stride of
// four floats per lane instead -- no pass through LDS, and every cache line is still used in full by the workgroup, but over four
// instructions: it takes 1.3 ... 1.6 times as long on an MI355X (tools/ab_dct.py); DCT_STAGED=0 in the Makefile builds it
// beside the shipped library.
//
// Twiddles: W_n^k (k < M) and W_4n^k (k <= M) are rows built at compile time from the fp64-rounded first octant of W_32768
// (smfft_twiddles_dct.inc, tools/gen_twiddles_dct.py) by exact symmetries (smfft_rows.hpp, which the four libraries of real rows on a
// half-length transform share), one row entry per element so that the lanes of a row read consecutive addresses.  No v_sin / v_cos.
//
// In place (d_out == d_in) is served: every value a workgroup loads from a row is consumed in front of the first exchange behind the
// loads -- the pass of the quads' second half through LDS, type III's partner exchange, or the transform's own; a barrier where a row
// spans waves -- and the stores come behind the transform; rows belong to one workgroup.
//
// Cache policy, by measurement: the 16-byte row accesses carry the engine's policy (non-temporal; -DSMFFT_NT=0
// builds them plain, -DSMFFT_DCT_NT_LOAD4 / -DSMFFT_DCT_NT_STORE4 one of them: the Makefile builds type III's stores plain at M = 2048,
// the one length where that form wins), the 4-byte ones -- type II's stores, type III's loads -- are plain (-DSMFFT_DCT_NT_STORE1=1 /
// -DSMFFT_DCT_NT_LOAD1=1 build them non-temporal: type II then takes 1.04 ... 1.6 times as long, type III up to 1.15 times, or ties).
//
// -ffp-contract=on (Makefile, DCT_FLAGS_<M>): a product is fused into a sum only where one expression of the source writes both, so
// every build of this file rounds alike and the A/B builds give the shipped build's bits; under hipcc's default (fast) the type III
// kernels of the two row-access forms differed in the last bit of 3.5 % of the outputs.
#include <hip/hip_runtime.h>

#include "smfft_dct.h"

namespace smfft {
namespace dct {
// enqueue `grid` workgroups on `stream`; 0 or the launch's hipError_t.  Defined per M by the objects compiled with -DSMFFT_DCT_N.
template <int M>
int launch_rows(const float* in, float* out, long long batch, int type, int sine, int grid, hipStream_t stream);
}  // namespace dct
}  // namespace smfft

#ifdef SMFFT_DCT_N
#include "smfft_fir_kernel.hpp"
#include "smfft_rows.hpp"

// 1: 16-byte row accesses and a pass through the row's LDS region; 0: 4-byte row accesses at stride four
#ifndef SMFFT_DCT_STAGED
#define SMFFT_DCT_STAGED 1
#endif

// the policy of the 16-byte row loads (type II) and stores (type III), and of the 4-byte row loads (type III) and stores (type II):
// 1 non-temporal, 0 plain
#ifndef SMFFT_DCT_NT_LOAD4
#define SMFFT_DCT_NT_LOAD4 SMFFT_NT
#endif
#ifndef SMFFT_DCT_NT_STORE4
#define SMFFT_DCT_NT_STORE4 SMFFT_NT
#endif
#ifndef SMFFT_DCT_NT_LOAD1
#define SMFFT_DCT_NT_LOAD1 0
#endif
#ifndef SMFFT_DCT_NT_STORE1
#define SMFFT_DCT_NT_STORE1 0
#endif

namespace smfft {
namespace dct {

using rows::w32768, rows::row_entry, rows::per_tile, rows::row_quad;

// the twiddle rows of n = 2 M points as (cos, sin), that is the CONJUGATES of W_n^k and W_4n^k
template <int M>
struct Rows {
    TwiddleValue wn[M];          // angle 2 pi k / n
    TwiddleValue w4[M + 1];      // angle 2 pi k / (4 n)
    constexpr Rows() : wn{}, w4{} {
        for (int k = 0; k < M; ++k) wn[k] = w32768(k * (16384 / M));
        for (int k = 0; k <= M; ++k) w4[k] = w32768(k * (4096 / M));
    }
};
template <int M>
static __device__ const Rows<M> rows = Rows<M>();

// one float, or four consecutive floats at 4-byte alignment, with the policies above
__device__ __forceinline__ float gload1(const float* p) { return rows::gload1<SMFFT_DCT_NT_LOAD1 != 0>(p); }
__device__ __forceinline__ void gstore1(float* p, float v) { rows::gstore1<SMFFT_DCT_NT_STORE1 != 0>(p, v); }
__device__ __forceinline__ row_quad gload4(const float* p) { return rows::gload4<SMFFT_DCT_NT_LOAD4 != 0>(p); }
__device__ __forceinline__ void gstore4(float* p, row_quad v) { rows::gstore4<SMFFT_DCT_NT_STORE4 != 0>(p, v); }

// out[r n + .] = DCT-II (sine == 0) or DST-II of in[r n + .], n = 2 M.  in and out may be the same buffer: no __restrict__.
template <int M>
__global__ void __launch_bounds__(kFirThreads) dct2_kernel(const float* in, float* out, long long batch, int sine) {
    using G = Geometry<M>;
    constexpr int T = G::T, n = 2 * M;
    __shared__ float2 s[G::kFftsPerBlock * G::SF];
    Engine<M, 0, 1> fwd;
    fwd.init(threadIdx.x);
    float2* sf = s + fwd.fft * G::SF;
    const long long ntiles = (batch + G::kFftsPerBlock - 1) / G::kFftsPerBlock;
    const bool self = fwd.u == 0;
    const float sign = sine ? -1.f : 1.f;      // of the odd samples, the second half of z
    const float cM = rows<M>.w4[M].x;          // cos(pi / 4)
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long g = tile * G::kFftsPerBlock + fwd.fft;
        const bool active = g < batch;
        // an inactive slot of the last tile reads row 0 and stores nothing
        const float* xr = in + (active ? g : 0) * n;
        float2 r[16], p[16];
#if SMFFT_DCT_STAGED
        row_quad f[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) f[q] = gload4(xr + 4 * (fwd.u + T * q));
        __builtin_amdgcn_sched_barrier(0);
        fft_sync<G::kMultiWave>();             // the previous tile's partner reads are done with the region
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            r[q] = make_float2(f[q].x, f[q].z);
            sf[M - 1 - (fwd.u + T * q)] = make_float2(sign * f[q].w, sign * f[q].y);     // z[M - 1 - p]
        }
        fft_sync<G::kMultiWave>();
#pragma unroll
        for (int q = 8; q < 16; ++q) r[q] = sf[fwd.u + T * q];
#else
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = fwd.u + T * q;
            const int i0 = q < 8 ? 4 * e : 2 * n - 1 - 4 * e;
            r[q] = make_float2(gload1(xr + i0), gload1(xr + (q < 8 ? i0 + 2 : i0 - 2)));
        }
        // nothing is scheduled across this point: the 32 loads all go out before the first arithmetic
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 8; q < 16; ++q) r[q] = make_float2(sign * r[q].x, sign * r[q].y);
#endif
        fft_sync<G::kMultiWave>();             // the region is free: the previous tile's partner reads, or the staging reads above
        fwd.transform(r, sf);
        fft_sync<G::kMultiWave>();             // the transform's last LDS reads are done
#pragma unroll
        for (int q = 0; q < 16; ++q) sf[fwd.u + T * q] = r[q];
        fft_sync<G::kMultiWave>();
        // Z[M - (u + T q)] = Z[(T - u) + T (15 - q)]; thread 0's q = 0 reads one element past the data, inside the region's padding, and
        // takes its own Z[0] instead
        const float2* partner = sf + (T - fwd.u);
#pragma unroll
        for (int q = 0; q < 16; ++q) p[q] = partner[T * (15 - q)];
        p[0] = self ? r[0] : p[0];
        float* yr = out + g * n;
        const int u = per_tile(fwd.u);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int k = fwd.u + T * q;
            const float2 wn = row_entry(&rows<M>.wn[u + T * q]), w4 = row_entry(&rows<M>.w4[u + T * q]);
            const float2 S = make_float2(r[q].x + p[q].x, r[q].y - p[q].y);       // Z + conj Z[M - k]
            const float2 D = make_float2(r[q].x - p[q].x, r[q].y + p[q].y);       // Z - conj Z[M - k]
            // V = S - i W_n^k D, W = (c, -s)
            const float vx = S.x + (wn.x * D.y - wn.y * D.x), vy = S.y - (wn.x * D.x + wn.y * D.y);
            // Y = W_4n^k V: X[k] = Re Y, X[n - k] = -Im Y
            float o0 = w4.x * vx + w4.y * vy, o1 = w4.y * vx - w4.x * vy;
            int k1 = n - k;
            if (q == 0) {
                // k = 0 has no X[n]: its thread stores X[M] = 2 W_4n^M (Re Z[0] - Im Z[0]) there
                o1 = self ? 2.f * (cM * (r[0].x - r[0].y)) : o1;
                k1 = self ? M : k1;
            }
            if (active) {
                gstore1(yr + (sine ? n - 1 - k : k), o0);
                gstore1(yr + (sine ? n - 1 - k1 : k1), o1);
            }
        }
    }
}

// out[r n + .] = DCT-III (sine == 0) or DST-III of in[r n + .], n = 2 M.  in and out may be the same buffer: no __restrict__.
template <int M>
__global__ void __launch_bounds__(kFirThreads) dct3_kernel(const float* in, float* out, long long batch, int sine) {
    using G = Geometry<M>;
    constexpr int T = G::T, n = 2 * M;
    __shared__ float2 s[G::kFftsPerBlock * G::SF];
    Engine<M, 1, 1> inv;
    inv.init(threadIdx.x);
    float2* sf = s + inv.fft * G::SF;
    const long long ntiles = (batch + G::kFftsPerBlock - 1) / G::kFftsPerBlock;
    const bool self = inv.u == 0;
    const float sign = sine ? -1.f : 1.f;      // of the odd samples, the second half of z
    const float2 wM = row_entry(&rows<M>.w4[M]);
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long g = tile * G::kFftsPerBlock + inv.fft;
        const bool active = g < batch;
        const float* xr = in + (active ? g : 0) * n;
        float a[16], b[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            // X[k] and X[n - k]; the sine transform reads the row reversed.  k = 0 has no X[n]: its thread reads X[M] there, for V'[M]
            const int k = inv.u + T * q;
            const int kb = (q == 0 && self) ? M : n - k;
            a[q] = gload1(xr + (sine ? n - 1 - k : k));
            b[q] = gload1(xr + (sine ? n - 1 - kb : kb));
        }
        // nothing is scheduled across this point: the 32 loads all go out before the first arithmetic
        __builtin_amdgcn_sched_barrier(0);
        const float xM = b[0];
        b[0] = self ? 0.f : b[0];
        const int u = per_tile(inv.u);
        float2 r[16], p[16];
        // V'[k] = conj(W_4n^k) (X[k] - i X[n - k]), conj(W) = (c, s)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float2 wk = row_entry(&rows<M>.w4[u + T * q]);
            r[q] = make_float2(wk.x * a[q] + wk.y * b[q], wk.y * a[q] - wk.x * b[q]);
        }
        fft_sync<G::kMultiWave>();             // the previous tile is done with the region
#pragma unroll
        for (int q = 0; q < 16; ++q) sf[inv.u + T * q] = r[q];
        // V'[M] = conj(W_4n^M) (X[M] - i X[M]) goes one element past the data, inside the region's padding: the partner of k = 0
        if (self) sf[M] = make_float2(wM.x * xM + wM.y * xM, wM.y * xM - wM.x * xM);
        fft_sync<G::kMultiWave>();
        // V'[M - (u + T q)] = V'[(T - u) + T (15 - q)]
        const float2* partner = sf + (T - inv.u);
#pragma unroll
        for (int q = 0; q < 16; ++q) p[q] = partner[T * (15 - q)];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float2 w = row_entry(&rows<M>.wn[u + T * q]);
            // A = V'[k] + conj V'[M - k], B = V'[k] - conj V'[M - k], Z = A + i conj(W_n^k) B
            const float2 A = make_float2(r[q].x + p[q].x, r[q].y - p[q].y), B = make_float2(r[q].x - p[q].x, r[q].y + p[q].y);
            r[q] = make_float2(A.x - (w.x * B.y + w.y * B.x), A.y + (w.x * B.x - w.y * B.y));
        }
        fft_sync<G::kMultiWave>();             // the partner reads are done
        inv.transform(r, sf);
        float* yr = out + g * n;
#if SMFFT_DCT_STAGED
        fft_sync<G::kMultiWave>();             // the transform's last LDS reads are done
#pragma unroll
        for (int q = 8; q < 16; ++q) sf[inv.u + T * q] = make_float2(sign * r[q].x, sign * r[q].y);
        fft_sync<G::kMultiWave>();
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = inv.u + T * q;
            const float2 m = sf[M - 1 - e];                                        // z[M - 1 - p]: y[4p + 3] + i y[4p + 1]
            const row_quad f = {r[q].x, m.y, r[q].y, m.x};
            if (active) gstore4(yr + 4 * e, f);
        }
#else
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = inv.u + T * q;
            const int i0 = q < 8 ? 4 * e : 2 * n - 1 - 4 * e;
            const float2 y = q < 8 ? r[q] : make_float2(sign * r[q].x, sign * r[q].y);
            if (active) {
                gstore1(yr + i0, y.x);
                gstore1(yr + (q < 8 ? i0 + 2 : i0 - 2), y.y);
            }
        }
#endif
    }
}

template <>
int launch_rows<SMFFT_DCT_N>(const float* in, float* out, long long batch, int type, int sine, int grid, hipStream_t stream) {
    if (type == 2) hipLaunchKernelGGL(dct2_kernel<SMFFT_DCT_N>, dim3((unsigned)grid), dim3(kFirThreads), 0, stream, in, out, batch, sine);
    else hipLaunchKernelGGL(dct3_kernel<SMFFT_DCT_N>, dim3((unsigned)grid), dim3(kFirThreads), 0, stream, in, out, batch, sine);
    return (int)hipGetLastError();
}

}  // namespace dct
}  // namespace smfft

#else  // the C ABI
#include "smfft_rows_host.hpp"

namespace {
// the launch of `grid` workgroups (<= 0: the default) on `stream`
auto dispatch(const void* in, void* out, int n, long long batch, int type, int sine) {
    return [=](int grid, hipStream_t stream) {
        const int M = half_length_fft_size(n);
        grid = default_grid(M, batch, grid);
        return dispatch_m(M, [&](auto m) { return smfft::dct::launch_rows<m()>((const float*)in, (float*)out, batch, type, sine != 0, grid, stream); });
    };
}

// -1: refused; 0: launch; 1: nothing to do.  No HIP call.  The output is the input (in place) or does not overlap it.
int check(const void* in, const void* out, int n, long long batch, int type) {
    if (half_length_fft_size(n) < 0 || (type != 2 && type != 3) || batch < 0) return -1;
    if (batch == 0) return 1;
    const unsigned long long count = (unsigned long long)batch * (unsigned long long)n;
    if (in != out && overlap(in, count, out, count)) return -1;
    return 0;
}
}  // namespace

extern "C" {

int smfft_dct_fft_size(int n) { return half_length_fft_size(n); }

int smfft_dct_launch(const void* d_in, void* d_out, int n, long long batch, int type, int sine, void* hip_stream) {
    return checked_launch(check(d_in, d_out, n, batch, type), dispatch(d_in, d_out, n, batch, type, sine), hip_stream);
}

int smfft_dct_launch_tuned(const void* d_in, void* d_out, int n, long long batch, int type, int sine, void* hip_stream, int grid) {
    return checked_launch_tuned(check(d_in, d_out, n, batch, type), dispatch(d_in, d_out, n, batch, type, sine), hip_stream, grid);
}

int smfft_dct_benchmark(const void* d_in, void* d_out, int n, long long batch, int type, int sine, double* FFT_time) {
    return checked_benchmark(check(d_in, d_out, n, batch, type), dispatch(d_in, d_out, n, batch, type, sine), FFT_time);
}

}  // extern "C"
#endif

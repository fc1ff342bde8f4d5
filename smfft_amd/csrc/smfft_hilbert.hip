// smfft_hilbert.hip -- libsmfft_hilbert.so: batched Hilbert transform, analytic signal and envelope of real rows of n = 512 ... 8192
// points (powers of two) on TWO complex transforms of M = n / 2 = 256 ... 4096 points of the register engine per row, in one kernel and
// one pass through HBM, and the C ABI of include/smfft_hilbert.h.
//
// Compiled once per M (Makefile: -DSMFFT_HILBERT_N=256 ... 4096, flags of their own: HILBERT_FLAGS_<M>) for the three kernels -- one per
// kind -- and their launcher, and once without SMFFT_HILBERT_N for the C ABI, which checks and dispatches.
//
// The geometry is dct2_kernel's (smfft_dct.hip: 256 threads, 4096 / M rows per workgroup, element u + T q in register q, workgroups
// stride over the tiles).  Consecutive pairs of samples are the two lanes of the transform, z[p] = x[2p] + i x[2p + 1]: one 8-byte load
// per element, consecutive lanes at consecutive addresses.
//     Z = DFT_M(z); partner P[k] = conj Z[(M - k) mod M] through the row's LDS region (the form of dct2_kernel);
//     Z'[k] = (conj(W_n^k) (Z[k] + P[k]) - W_n^k (Z[k] - P[k])) / n, Z'[0] = 0, W_n = exp(-2 pi i / n).  With W_n^k = c - i s this is
//           = (2 / n) (c P[k] + i s Z[k]): two products per component, and that is how it is computed;
//     z' = the un-normalised inverse DFT_M(Z'); H(x)[2p] = Re z'[p], H(x)[2p + 1] = Im z'[p].
// The Hermitian split of Z into the spectra of the even and the odd samples, the multiplier -i s[k] of the n-point spectrum, its zeroed
// bins 0 and n / 2 (both live in Z[0]) and the merge in front of a C2R transform are that one line.  2 / n is a power of two: exact.
//
// Kinds (the template parameter KIND): 0 stores H(x) (one 8-byte store per element), 1 stores x + i H(x) (one 16-byte store
// (x[2p], H[2p], x[2p + 1], H[2p + 1]) per element), 2 stores sqrt(x^2 + H(x)^2) (8 bytes).  Kinds 1 and 2 need x again at the store:
// the sixteen loaded pairs stay in registers across both transforms.  -DSMFFT_HILBERT_KEEP_X=0 builds the other form, which loads them
// a second time behind the inverse transform -- all sixteen loads, by the thread that stores those very elements, in front of its
// first store; it takes 1.1 ... 1.3 times as long on an MI355X (tools/ab_hilbert.py).
//
// Twiddles: W_n^k (k < M) is the row that the DCT kernels build at compile time from the fp64-rounded first octant of W_32768
// (smfft_twiddles_dct.inc) by exact symmetries (smfft_rows.hpp), in an object of this library's own so that smfft_dct.hip and its ten
// kernels stay as they are.  No v_sin / v_cos.
//
// In place (d_out == d_in), kinds 0 and 2: every value a workgroup loads from a row is consumed in front of the first exchange behind
// the loads (the forward transform's own; a barrier where a row spans waves) and the stores come behind the inverse transform; rows
// belong to one workgroup.  (In the build with the second load of x, kind 2's argument is the thread's own: it loads exactly the
// sixteen pairs that it then overwrites, every load in front of the first store, and no other thread touches them.)  Kind 1's output is
// twice the input: any overlap is refused.
//
// -ffp-contract=on (Makefile, HILBERT_FLAGS_<M>): a product is fused into a sum only where one expression of the source writes both,
// so every build of this file rounds alike and the A/B builds give the shipped build's bits (the reason of DCT_FLAGS).
#include <hip/hip_runtime.h>

#include "smfft_hilbert.h"

namespace smfft {
namespace hilbert {
// enqueue `grid` workgroups on `stream`; 0 or the launch's hipError_t.  Defined per M by the objects compiled with -DSMFFT_HILBERT_N.
template <int M>
int launch_rows(const float* in, float* out, long long batch, int kind, int grid, hipStream_t stream);
}  // namespace hilbert
}  // namespace smfft

#ifdef SMFFT_HILBERT_N
#include "smfft_fir_kernel.hpp"
#include "smfft_rows.hpp"

// kinds 1 and 2: 1 keeps x in registers across the transforms, 0 loads it a second time in front of the store.  Both stay under 256
// VGPRs without scratch; kept ships by measurement (the second load costs 10 ... 32 % of the launch)
#ifndef SMFFT_HILBERT_KEEP_X
#define SMFFT_HILBERT_KEEP_X 1
#endif
// the policy of the row loads and of the stores: 1 non-temporal, 0 plain
#ifndef SMFFT_HILBERT_NT_LOAD
#define SMFFT_HILBERT_NT_LOAD SMFFT_NT
#endif
#ifndef SMFFT_HILBERT_NT_STORE
#define SMFFT_HILBERT_NT_STORE SMFFT_NT
#endif

namespace smfft {
namespace hilbert {

using rows::w32768, rows::row_entry, rows::per_tile, rows::row_quad;

// the twiddle row of n = 2 M points as (cos, sin)(2 pi k / n), that is the CONJUGATE of W_n^k
template <int M>
struct Rows {
    TwiddleValue wn[M];
    constexpr Rows() : wn{} {
        for (int k = 0; k < M; ++k) wn[k] = w32768(k * (16384 / M));
    }
};
template <int M>
static __device__ const Rows<M> rows = Rows<M>();

// two or four consecutive floats at 4-byte alignment, with the policies above
__device__ __forceinline__ float2 gload2(const float* p) { return rows::gload2<SMFFT_HILBERT_NT_LOAD != 0>(p); }
__device__ __forceinline__ void gstore2(float* p, float a, float b) { rows::gstore2<SMFFT_HILBERT_NT_STORE != 0>(p, a, b); }
__device__ __forceinline__ void gstore4(float* p, row_quad v) { rows::gstore4<SMFFT_HILBERT_NT_STORE != 0>(p, v); }
// a loaded pair as two values of their own.  Where the pairs are kept across the transforms (x below), the compiler otherwise holds
// them as the vectors they were loaded as and runs the forward transform's first additions on those: thirty v_pk_add_f32 per thread,
// half rate on gfx950, whatever -fno-slp-vectorize says
__device__ __forceinline__ float2 taken_apart(float2 v) {
    asm volatile("" : "+v"(v.x), "+v"(v.y));
    return v;
}

// KIND 0: out[r n + .] = H(in[r n + .]); 1: out[2 (r n + j)], out[2 (r n + j) + 1] = in[r n + j], H(in[r n + .])[j];
// 2: out[r n + j] = sqrt(in[r n + j]^2 + H(in[r n + .])[j]^2); n = 2 M.  Kinds 0 and 2: in and out may be the same buffer, no
// __restrict__.
template <int M, int KIND>
__global__ void __launch_bounds__(kFirThreads) hilbert_kernel(const float* in, float* out, long long batch) {
    using G = Geometry<M>;
    constexpr int T = G::T, n = 2 * M;
    constexpr bool kNeedsX = KIND != 0, kKeepX = kNeedsX && SMFFT_HILBERT_KEEP_X != 0;
    __shared__ float2 s[G::kFftsPerBlock * G::SF];
    Engine<M, 0, 1> fwd;
    Engine<M, 1, 1> inv;
    fwd.init(threadIdx.x);
    inv.init(threadIdx.x);
    float2* sf = s + fwd.fft * G::SF;
    const long long ntiles = (batch + G::kFftsPerBlock - 1) / G::kFftsPerBlock;
    const bool self = fwd.u == 0;
    const float scale = 1.f / (float)M;        // 2 / n: the inverse transform is un-normalised.  An exact power of two
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long g = tile * G::kFftsPerBlock + fwd.fft;
        const bool active = g < batch;
        // an inactive slot of the last tile reads row 0 and stores nothing
        const float* xr = in + (active ? g : 0) * n;
        float2 r[16], p[16];
        [[maybe_unused]] float2 x[kNeedsX ? 16 : 1];
#pragma unroll
        for (int q = 0; q < 16; ++q) r[q] = gload2(xr + 2 * (fwd.u + T * q));
        // nothing is scheduled across this point: the sixteen loads all go out before the first arithmetic
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (kKeepX) {
#pragma unroll
            for (int q = 0; q < 16; ++q) x[q] = r[q] = taken_apart(r[q]);
        }
        fft_sync<G::kMultiWave>();             // the previous tile's inverse transform is done with the region
        fwd.transform(r, sf);
        fft_sync<G::kMultiWave>();             // the transform's last LDS reads are done
#pragma unroll
        for (int q = 0; q < 16; ++q) sf[fwd.u + T * q] = r[q];
        fft_sync<G::kMultiWave>();
        // Z[M - (u + T q)] = Z[(T - u) + T (15 - q)]; thread 0's q = 0 reads one element past the data, inside the region's padding: its
        // Z'[0] is zero whatever it read
        const float2* partner = sf + (T - fwd.u);
#pragma unroll
        for (int q = 0; q < 16; ++q) p[q] = partner[T * (15 - q)];
        const int u = per_tile(fwd.u);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float2 w = row_entry(&rows<M>.wn[u + T * q]);        // (c, s): W_n^k = c - i s
            // Z' = (2 / n) (c conj Z[M - k] + i s Z[k])
            r[q] = make_float2(scale * (w.x * p[q].x - w.y * r[q].y), scale * (w.y * r[q].x - w.x * p[q].y));
        }
        r[0] = self ? make_float2(0.f, 0.f) : r[0];       // bins 0 and n / 2 of the row's spectrum
        fft_sync<G::kMultiWave>();             // the partner reads are done
        inv.transform(r, sf);
        if constexpr (kNeedsX && !kKeepX) {
#pragma unroll
            for (int q = 0; q < 16; ++q) x[q] = gload2(xr + 2 * (fwd.u + T * q));
            // every load of the thread's elements is out before its first store (in place, kind 2)
            __builtin_amdgcn_sched_barrier(0);
        }
        float* yr = out + g * (KIND == 1 ? 2 * n : n);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = fwd.u + T * q;
            if constexpr (KIND == 0) {
                if (active) gstore2(yr + 2 * e, r[q].x, r[q].y);
            } else if constexpr (KIND == 1) {
                const row_quad f = {x[q].x, r[q].x, x[q].y, r[q].y};
                if (active) gstore4(yr + 4 * e, f);
            } else {
                const float e0 = sqrtf(x[q].x * x[q].x + r[q].x * r[q].x), e1 = sqrtf(x[q].y * x[q].y + r[q].y * r[q].y);
                if (active) gstore2(yr + 2 * e, e0, e1);
            }
        }
    }
}

template <>
int launch_rows<SMFFT_HILBERT_N>(const float* in, float* out, long long batch, int kind, int grid, hipStream_t stream) {
    const dim3 blocks((unsigned)grid), threads(kFirThreads);
    if (kind == 0) hipLaunchKernelGGL((hilbert_kernel<SMFFT_HILBERT_N, 0>), blocks, threads, 0, stream, in, out, batch);
    else if (kind == 1) hipLaunchKernelGGL((hilbert_kernel<SMFFT_HILBERT_N, 1>), blocks, threads, 0, stream, in, out, batch);
    else hipLaunchKernelGGL((hilbert_kernel<SMFFT_HILBERT_N, 2>), blocks, threads, 0, stream, in, out, batch);
    return (int)hipGetLastError();
}

}  // namespace hilbert
}  // namespace smfft

#else  // the C ABI
#include "smfft_rows_host.hpp"

namespace {
// the launch of `grid` workgroups (<= 0: the default) on `stream`
auto dispatch(const void* in, void* out, int n, long long batch, int kind) {
    return [=](int grid, hipStream_t stream) {
        const int M = half_length_fft_size(n);
        grid = default_grid(M, batch, grid);
        return dispatch_m(M, [&](auto m) { return smfft::hilbert::launch_rows<m()>((const float*)in, (float*)out, batch, kind, grid, stream); });
    };
}

// -1: refused; 0: launch; 1: nothing to do.  No HIP call.  Kinds 0 and 2: the output is the input (in place) or does not overlap it;
// kind 1: it does not overlap it
int check(const void* in, const void* out, int n, long long batch, int kind) {
    if (half_length_fft_size(n) < 0 || kind < 0 || kind > 2 || batch < 0) return -1;
    if (batch == 0) return 1;
    const unsigned long long ins = (unsigned long long)batch * (unsigned long long)n;
    if (in == out) return kind == 1 ? -1 : 0;
    if (overlap(in, ins, out, kind == 1 ? 2 * ins : ins)) return -1;
    return 0;
}
}  // namespace

extern "C" {

int smfft_hilbert_fft_size(int n) { return half_length_fft_size(n); }

int smfft_hilbert_launch(const void* d_in, void* d_out, int n, long long batch, int kind, void* hip_stream) {
    return checked_launch(check(d_in, d_out, n, batch, kind), dispatch(d_in, d_out, n, batch, kind), hip_stream);
}

int smfft_hilbert_launch_tuned(const void* d_in, void* d_out, int n, long long batch, int kind, void* hip_stream, int grid) {
    return checked_launch_tuned(check(d_in, d_out, n, batch, kind), dispatch(d_in, d_out, n, batch, kind), hip_stream, grid);
}

int smfft_hilbert_benchmark(const void* d_in, void* d_out, int n, long long batch, int kind, double* FFT_time) {
    return checked_benchmark(check(d_in, d_out, n, batch, kind), dispatch(d_in, d_out, n, batch, kind), FFT_time);
}

}  // extern "C"
#endif

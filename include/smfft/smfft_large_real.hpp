// smfft_large_real.hpp -- single-pass R2C / C2R of real N = 16384 and 32768 (gfx950), on the C2C engine of smfft_large.hpp.
//
// A real FFT of length N = 2L is a complex FFT of length L plus a Hermitian split (R2C) or merge (C2R).  L = 8192 / 16384 are the
// lengths LargeEngine<L, DIR> transforms whole in one workgroup's LDS, so each real FFT is one HBM read and one HBM write of N * 4
// bytes.  The engine and its geometry are used as they are; what is added (tools/large_real_model.py replays it in fp64 and counts
// its bank conflicts):
//
//   * R2C: z[n] = x[2n] + i x[2n+1] is the input viewed as float2; the four passes give thread u Z[u + T*q], q < 16, T = L/16.
//     Exchange S, through the same LDS image: Z[u + T*q] is written at its natural index, a barrier, the partner Z[(L - k) mod L]
//     of k = u + T*q is read (lanes read consecutive addresses in descending order: conflict free), a barrier (the image is free
//     for the next FFT's exchange A).  Then X[k] = S/2 + V D, S = Z[k] + conj Z[L-k], D = Z[k] - conj Z[L-k], V = -(i/2) W_N^k,
//     stored coalesced to out[u + T*q] in the packed layout: element 0 = (X[0], X[L]) = (Re Z0 + Im Z0, Re Z0 - Im Z0).
//   * C2R: thread u loads P[u + T*c]; exchange S as above; Z[k] = S/2 + V D with V = (i/2) conj W_N^k (element 0: Z[0] =
//     (P0.re + P0.im, P0.re - P0.im) / 2, X[0] = P0.re and X[L] = P0.im taken as real); the four inverse passes give L z, stored
//     as N floats: (N/2) x.
//   * Twiddles: V for k = u + T*q is V_u * W_32^{+-q}: one row V_u = -+(i/2) W_N^{+-u} per N and direction, rebuilt at compile time
//     from the fp64-rounded W_32768^m, m < 1024 (smfft_twiddles_32768.inc; W_16384^u = W_32768^{2u}), loaded once per thread
//     before the persistent loop (two VGPRs); W_32^q = W_16384^{512 q}, exact entries of the W_16384 table, are compile-time
//     constants.  The halving and the quarter turn are exact, so V_u is correctly rounded too.
//   * Barriers per FFT: the six of the C2C loop and the two of exchange S.  LDS: the C2C image of L (64.25 / 128.25 KiB).
//
// Buffer contract (include/smfft.h): 8-byte-aligned pointers, 64-bit element offsets, only FFTs [0, nFFTs) read or written,
// d_output == d_input allowed (a workgroup reads all of an FFT before it writes any of it, and both sides are N * 4 bytes), no
// partial overlap.
#pragma once
#include <hip/hip_runtime.h>
#include "smfft_large.hpp"

namespace smfft {
namespace large {

// (cos, sin)(2 pi m / 32768), m < 1024
static constexpr TwiddleValue row_32768[1024] = {
#include "smfft_twiddles_32768.inc"
};

template <int N>
struct LargeRealGeometry {
    static_assert(N == 16384 || N == 32768, "the single-pass real transforms serve N = 16384 and 32768");
    static constexpr int L = N / 2;                    // the complex length
    using G = LargeGeometry<L>;
    static constexpr int T = G::T;                     // threads per FFT
    static_assert(32 * T == N, "k = u + T*q: W_N^k = W_N^u W_32^q");
    static_assert(G::kLdsFloat2 > L, "exchange S also writes element 0 at L");
    // exchange S: element p lives at p; the partner of element p, and where it is read (element 0's own copy sits at L)
    __host__ __device__ static constexpr int partner(int p) { return (L - p) & (L - 1); }
    __host__ __device__ static constexpr int partner_slot(int p) { return L - p; }
};

// the split (DIR = 0) / merge (DIR = 1) row: v[u] = -(i/2) W_N^u (DIR 0) or (i/2) conj W_N^u (DIR 1), u < T, and the factors
// w32[q] = W_32^q (DIR 0) or conj W_32^q (DIR 1) that give V for element u + T*q: v[u] * w32[q]
template <int N, int DIR>
struct LargeRealTwiddles {
    using RG = LargeRealGeometry<N>;
    TwiddleValue v[RG::T];
    TwiddleValue w32[16];
    constexpr LargeRealTwiddles() : v{}, w32{} {
        for (int u = 0; u < RG::T; ++u) {
            const TwiddleValue cs = row_32768[u * (32768 / N)];        // (cos, sin) of 2 pi u / N
            // W = (c, -s): -(i/2) W = (-s, -c) / 2;  (i/2) conj W = (-s, c) / 2
            v[u] = TwiddleValue{-0.5f * cs.y, DIR ? 0.5f * cs.x : -0.5f * cs.x};
        }
        for (int q = 0; q < 16; ++q) {
            const TwiddleValue w = w16384(512 * q);
            w32[q] = TwiddleValue{w.x, DIR ? -w.y : w.y};
        }
    }
};
template <int N, int DIR>
static __device__ const LargeRealTwiddles<N, DIR> large_real_twiddles = LargeRealTwiddles<N, DIR>();

// ------------------------------------------------------------------------------------------------
// Exchange S and the split / merge of one thread's 16 elements u + T*q.  u = threadIdx.x; lds = the workgroup's image.
// ------------------------------------------------------------------------------------------------
template <int N, int DIR>
struct LargeRealSplit {
    using RG = LargeRealGeometry<N>;
    static constexpr int L = RG::L, T = RG::T;
    static constexpr LargeRealTwiddles<N, DIR> kRows = LargeRealTwiddles<N, DIR>();
    typedef __attribute__((address_space(1))) const LargeRealTwiddles<N, DIR> GlobalRow;
    int u;

    __device__ __forceinline__ explicit LargeRealSplit(int tid) : u(tid) {}

    // V_u of this thread (one global load)
    __device__ __forceinline__ float2 row() const {
        GlobalRow* t = (GlobalRow*)&large_real_twiddles<N, DIR>;
        const float x = t->v[u].x, y = t->v[u].y;
        return make_float2(x, y);
    }
    // element u + T*q at u + T*q; thread 0 also puts element 0 at L, one past the end (the image holds L + 32 float2), so that every
    // partner read below is one base register and a constant offset: L - u - T*q = (T - u) + T*(15 - q), and L for element 0
    __device__ __forceinline__ void write(const float2 (&a)[16], float2* lds) const {
#pragma unroll
        for (int q = 0; q < 16; ++q) lds[u + T * q] = a[q];
        if (u == 0) lds[L] = a[0];
    }
    __device__ __forceinline__ void read_partner(float2 (&b)[16], const float2* lds) const {
        const float2* base = lds + (T - u);
#pragma unroll
        for (int q = 0; q < 16; ++q) b[q] = base[T * (15 - q)];
    }
    // a[q] <- S/2 + V D, S = a + conj b, D = a - conj b, V = vu * w32[q]; element 0 (u = 0, q = 0) by its own rule
    __device__ __forceinline__ void apply(float2 (&a)[16], const float2 (&b)[16], float2 vu) const {
        const float2 a0 = a[0];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float2 v = q == 0 ? vu : cmul(vu, make_float2(kRows.w32[q].x, kRows.w32[q].y));
            const float sx = a[q].x + b[q].x, sy = a[q].y - b[q].y;
            const float dx = a[q].x - b[q].x, dy = a[q].y + b[q].y;
            a[q] = make_float2(0.5f * sx + (v.x * dx - v.y * dy), 0.5f * sy + (v.x * dy + v.y * dx));
        }
        if (u == 0) {
            const float s = a0.x + a0.y, d = a0.x - a0.y;
            a[0] = DIR ? make_float2(0.5f * s, 0.5f * d) : make_float2(s, d);
        }
    }
};

// ------------------------------------------------------------------------------------------------
// The kernels: a persistent grid, FFT f = blockIdx.x, blockIdx.x + gridDim.x, ... < nFFTs, as large_c2c.  N is the real length.
// ------------------------------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(N / 32) __attribute__((amdgpu_waves_per_eu(4))) void large_r2c(const float* d_input, float2* d_output, int nFFTs) {
    constexpr int L = N / 2;
    using G = LargeGeometry<L>;
    __shared__ float2 lds[G::kLdsFloat2];
    LargeEngine<L, 0> e(threadIdx.x);
    LargeRealSplit<N, 0> s(threadIdx.x);
    const float2* in = (const float2*)d_input;
    long f = blockIdx.x;
    if (f >= nFFTs) return;
    const float2 vu = s.row();
    float2 r[16], y[16];
    for (;;) {
        const long next = f + gridDim.x;
        e.reload_twiddles();
        e.load(r, in + f * L);
        large_transform<L, 0>(e, r, y, lds);      // its last barrier frees the image for exchange S
        float2 v[16];
        s.write(y, lds);
        __syncthreads();
        s.read_partner(v, lds);
        __syncthreads();      // the image is free for the next FFT's exchange A
        s.apply(y, v, vu);
        e.store(y, d_output + f * L);
        if (next >= nFFTs) break;
        f = next;
    }
}

template <int N>
__global__ __launch_bounds__(N / 32) __attribute__((amdgpu_waves_per_eu(4))) void large_c2r(const float2* d_input, float* d_output, int nFFTs) {
    constexpr int L = N / 2;
    using G = LargeGeometry<L>;
    __shared__ float2 lds[G::kLdsFloat2];
    LargeEngine<L, 1> e(threadIdx.x);
    LargeRealSplit<N, 1> s(threadIdx.x);
    float2* out = (float2*)d_output;
    long f = blockIdx.x;
    if (f >= nFFTs) return;
    const float2 vu = s.row();
    float2 r[16], y[16];
    for (;;) {
        const long next = f + gridDim.x;
        e.reload_twiddles();
        e.load(r, d_input + f * L);
        s.write(r, lds);
        __syncthreads();
        s.read_partner(y, lds);
        __syncthreads();      // the image is free for exchange A
        s.apply(r, y, vu);
        large_transform<L, 1>(e, r, y, lds);      // its last barrier frees the image for the next FFT's exchange S
        e.store(y, out + f * L);
        if (next >= nFFTs) break;
        f = next;
    }
}

}  // namespace large
}  // namespace smfft

// smfft_large.hpp -- the single-pass C2C engine of N = 8192 and 16384 (gfx950: 160 KiB of LDS per CU).
//
// One workgroup transforms one whole FFT at a time: one HBM read of the input straight into registers, every pass on chip, one HBM
// write of the output straight from registers -- the shape of the N <= 4096 external kernels, at lengths whose complex fp32 image
// (64 / 128 KiB) fits one CU's LDS.  The plan (tools/large_plan_model.py replays it in fp64 and counts its bank conflicts):
//
//   * N = 16 * 16 * R * 16, R = N / 4096; 16 elements per thread, T = N / 16 threads (8 / 16 waves).
//   * A four-pass Stockham autosort, decimation in time.  Pass (radix r, span Ns) runs butterfly j on x[j + i*N/r], i < r,
//     multiplies by W_{Ns*r}^{i*(j mod Ns)}, and writes y[(j / Ns)*Ns*r + (j mod Ns) + i*Ns]; (r, Ns) = (16, 1), (16, 16), (R, 256),
//     (16, N/16).  Natural order in and out: the digit reversal is folded into the addressing.
//   * Pass 1 reads global memory (x[u + T*c]: consecutive threads, consecutive elements) and pass 4 writes it (y[u + T*q]); the
//     three exchanges between them go through one LDS image.  Only exchange A (pass 1 -> 2) needs padding: element p = 16a + b at
//     b*SA + a with SA = T + 2, so that pass 1's writes (lane u -> b*SA + u) are distinct mod 16 in every 16-lane group and pass
//     2's reads (u -> (u mod 16)*SA + u/16 + const) distinct mod 32 in every 32-lane group.  Exchanges B and C are conflict free
//     in natural order.  Image: 16 * SA float2 = N*8 + 256 B: 64.25 KiB (two workgroups per CU) / 128.25 KiB (one).
//   * One region serves all three exchanges, so each is a write, a barrier, a read and a barrier: six barriers per FFT (large_transform).
//   * Twiddles: per-N rows built at compile time from the fp64-rounded W_16384 octant (smfft_twiddles_16384.inc), so that the
//     threads of a wave read consecutive (pass 4) or few (passes 2, 3) addresses; they are loaded per FFT from L2, not kept in
//     VGPRs across the persistent loop, which keeps the kernel under 128 VGPRs (4 waves per SIMD) without scratch.
//   * Persistent grid (one or two workgroups per CU), grid-stride over FFTs; each FFT's loads are issued at the top of its
//     iteration.  (A form that loaded the next FFT before the current one's last exchange was tried: on the MI355X it returned
//     wrong results for every FFT but those of the last round of the grid, and was dropped -- DESIGN.md section 9.)
//
// Buffer contract (include/smfft.h): 8-byte-aligned pointers, 64-bit element offsets, only FFTs [0, nFFTs) read or written,
// d_output == d_input allowed (a workgroup reads all of an FFT before it writes any of it), no partial overlap.
#pragma once
#include <hip/hip_runtime.h>
#include "smfft_engine.hpp"

namespace smfft {
namespace large {

// ------------------------------------------------------------------------------------------------
// W_16384^m = (cos, -sin)(2 pi m / 16384), rebuilt from the first octant by exact symmetries
// ------------------------------------------------------------------------------------------------
static constexpr int kTable = 16384;
static constexpr TwiddleValue octant_16384[kTable / 8 + 1] = {
#include "smfft_twiddles_16384.inc"
};
constexpr TwiddleValue w16384(int m) {
    m &= kTable - 1;
    const int q = m / (kTable / 4), r = m % (kTable / 4);
    const TwiddleValue o = r <= kTable / 8 ? octant_16384[r] : TwiddleValue{octant_16384[kTable / 4 - r].y, octant_16384[kTable / 4 - r].x};
    // (cos, sin) of q quarter turns + the octant's angle
    const float c = q == 0 ? o.x : q == 1 ? -o.y : q == 2 ? -o.x : o.y;
    const float s = q == 0 ? o.y : q == 1 ? o.x : q == 2 ? -o.y : -o.x;
    return TwiddleValue{c, -s};
}

// ------------------------------------------------------------------------------------------------
template <int N>
struct LargeGeometry {
    static_assert(N == 8192 || N == 16384, "the single-pass large engine serves N = 8192 and 16384");
    static constexpr int T = N / 16;                   // threads per FFT (= per workgroup)
    static constexpr int R = N / 4096;                 // radix of pass 3
    static constexpr int B3 = 16 / R;                  // pass-3 butterflies per thread
    static constexpr int SA = T + 2;                   // row stride of exchange A
    static constexpr int kLdsFloat2 = 16 * SA;         // the LDS image
    static constexpr int kLdsBytes = 8 * kLdsFloat2;
    static constexpr int kWorkgroupsPerCu = 163840 / kLdsBytes;
    static_assert(kWorkgroupsPerCu == (N == 8192 ? 2 : 1), "LDS budget");
    // exchange A: physical float2 index of logical element p
    __host__ __device__ static constexpr int lds_a(int p) { return (p % 16) * SA + p / 16; }
};

// the twiddle rows (powers of W_16384): w2[(i-1)*16 + k] = W_256^{i*k}, w3[(i-1)*256 + k] = W_{256R}^{i*k}, w4[(i-1)*T + u] = W_N^{i*u}
template <int N>
struct LargeTwiddleRows {
    using G = LargeGeometry<N>;
    TwiddleValue w2[15 * 16];
    TwiddleValue w3[(G::R - 1) * 256];
    TwiddleValue w4[15 * G::T];
    constexpr LargeTwiddleRows() : w2{}, w3{}, w4{} {
        for (int i = 1; i < 16; ++i)
            for (int k = 0; k < 16; ++k) w2[(i - 1) * 16 + k] = w16384(i * k * (kTable / 256));
        for (int i = 1; i < G::R; ++i)
            for (int k = 0; k < 256; ++k) w3[(i - 1) * 256 + k] = w16384(i * k * (kTable / (256 * G::R)));
        for (int i = 1; i < 16; ++i)
            for (int u = 0; u < G::T; ++u) w4[(i - 1) * G::T + u] = w16384(i * u * (kTable / N));
    }
};
template <int N>
static __device__ const LargeTwiddleRows<N> large_twiddle_rows = LargeTwiddleRows<N>();

typedef __attribute__((address_space(1))) const TwiddleValue GlobalTwiddle;
template <int DIR>
__device__ __forceinline__ float2 twiddle_at(GlobalTwiddle* p) {
    const float x = p->x, y = p->y;
    return make_float2(x, DIR ? -y : y);
}

// ------------------------------------------------------------------------------------------------
// One thread's part of one FFT.  u = threadIdx.x; lds = the workgroup's image.
// ------------------------------------------------------------------------------------------------
template <int N, int DIR>
struct LargeEngine {
    using G = LargeGeometry<N>;
    static constexpr int T = G::T, R = G::R, B3 = G::B3, SA = G::SA;
    typedef __attribute__((address_space(1))) const LargeTwiddleRows<N> GlobalRows;
    int u;
    GlobalRows* rows;      // a global-address-space pointer: global_load, not flat_load (which also counts as an LDS access)

    __device__ __forceinline__ explicit LargeEngine(int tid) : u(tid), rows((GlobalRows*)&large_twiddle_rows<N>) {}
    // Called once per FFT: hides the (uniform) address of the twiddle rows from the optimiser, so that it cannot hoist the 33
    // loop-invariant twiddle loads out of the persistent loop -- kept live across it they take ~66 VGPRs and spill.
    __device__ __forceinline__ void reload_twiddles() { asm volatile("" : "+s"(rows)); }

    __device__ __forceinline__ void load(float2 (&r)[16], const float2* g) const {
#pragma unroll
        for (int c = 0; c < 16; ++c) r[c] = gload(g + u + T * c);
    }
    __device__ __forceinline__ void store(const float2 (&r)[16], float2* g) const {
#pragma unroll
        for (int q = 0; q < 16; ++q) gstore(g + u + T * q, r[q]);
    }

    // pass 1 (radix 16, span 1) and the write of exchange A: element 16u + q at q*SA + u
    __device__ __forceinline__ void pass1_write(const float2 (&r)[16], float2* lds) const {
        float2 y[16];
        SmallDft<16, 1, DIR>::run(r, y);
#pragma unroll
        for (int q = 0; q < 16; ++q) lds[q * SA + u] = y[q];
    }
    // exchange A's read (element u + T*i) and pass 2 (radix 16, span 16): y[q] goes to (u/16)*256 + u%16 + 16q
    __device__ __forceinline__ void read_pass2(float2 (&y)[16], const float2* lds) const {
        const float2* base = lds + G::lds_a(u);
        float2 v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = base[(T / 16) * i];
        GlobalTwiddle* w = rows->w2 + (u & 15);
#pragma unroll
        for (int i = 1; i < 16; ++i) v[i] = cmul(v[i], twiddle_at<DIR>(w + (i - 1) * 16));
        SmallDft<16, 1, DIR>::run(v, y);
    }
    __device__ __forceinline__ void write_b(const float2 (&y)[16], float2* lds) const {
        float2* base = lds + (u >> 4) * 256 + (u & 15);
#pragma unroll
        for (int q = 0; q < 16; ++q) base[16 * q] = y[q];
    }
    // exchange B's read and pass 3 (radix R, span 256): butterfly j = u + T*b reads j + (N/R)*i, y[b*R + q] goes to
    // (j/256)*256R + j%256 + 256q
    __device__ __forceinline__ void read_pass3(float2 (&y)[16], const float2* lds) const {
        const float2* base = lds + u;
        GlobalTwiddle* w = rows->w3 + (u & 255);
        float2 tw[R];
#pragma unroll
        for (int i = 1; i < R; ++i) tw[i] = twiddle_at<DIR>(w + (i - 1) * 256);
#pragma unroll
        for (int b = 0; b < B3; ++b) {
            float2 v[R];
#pragma unroll
            for (int i = 0; i < R; ++i) v[i] = base[T * b + (N / R) * i];
#pragma unroll
            for (int i = 1; i < R; ++i) v[i] = cmul(v[i], tw[i]);
            SmallDft<R, 1, DIR>::run(v, &y[b * R]);
        }
    }
    __device__ __forceinline__ void write_c(const float2 (&y)[16], float2* lds) const {
        float2* base = lds + (u >> 8) * (256 * R) + (u & 255);
#pragma unroll
        for (int b = 0; b < B3; ++b)
#pragma unroll
            for (int q = 0; q < R; ++q) base[(T / 256) * b * (256 * R) + 256 * q] = y[b * R + q];
    }
    // exchange C's read (element u + T*i) and pass 4 (radix 16, span N/16): y[q] = X[u + T*q]
    __device__ __forceinline__ void read_c(float2 (&v)[16], const float2* lds) const {
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = lds[u + T * i];
    }
    __device__ __forceinline__ void pass4(float2 (&v)[16], float2 (&y)[16]) const {
        GlobalTwiddle* w = rows->w4 + u;
#pragma unroll
        for (int i = 1; i < 16; ++i) v[i] = cmul(v[i], twiddle_at<DIR>(w + (i - 1) * T));
        SmallDft<16, 1, DIR>::run(v, y);
    }
};

// the six barriers and four passes between a thread's sixteen inputs r[c] = x[u + T*c] and its outputs y[q] = X[u + T*q]
template <int N, int DIR>
__device__ __forceinline__ void large_transform(const LargeEngine<N, DIR>& e, float2 (&r)[16], float2 (&y)[16], float2* lds) {
    e.pass1_write(r, lds);
    __syncthreads();
    e.read_pass2(y, lds);
    __syncthreads();
    e.write_b(y, lds);
    __syncthreads();
    e.read_pass3(y, lds);
    __syncthreads();
    e.write_c(y, lds);
    __syncthreads();
    float2 v[16];
    e.read_c(v, lds);
    __syncthreads();      // the image is free for the caller's next exchange
    e.pass4(v, y);
}

// ------------------------------------------------------------------------------------------------
// Uniform values in scalar registers, for the kernels whose addresses are a per-workgroup base and a 32-bit lane offset
// ------------------------------------------------------------------------------------------------
typedef __attribute__((address_space(1))) const float2 GlobalFloat2;

// a value that is the same in every lane, moved to a scalar register (a 32-bit division leaves its uniform quotient in a vector one,
// and everything derived from it -- base pointers, bounds -- would follow it there)
__device__ __forceinline__ unsigned uniform(unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (unsigned)__builtin_amdgcn_readfirstlane((int)v);
#else
    return v;
#endif
}
__device__ __forceinline__ long long uniform(long long v) {
    return (long long)(((unsigned long long)uniform((unsigned)((unsigned long long)v >> 32)) << 32) | uniform((unsigned)v));
}

// A uniform pointer, pinned to a scalar register pair (and hidden from the optimiser): a load through it takes the scalar base and one
// 32-bit lane offset.  Left alone, the sixteen row addresses of a tap -- too far apart for the instruction's immediate offset -- become
// sixteen 64-bit vector additions per row, or vector pointers carried round the tap loop.  The pointer must be the same in every lane:
// for one that is not, the compiler silently takes the first active lane's (a readfirstlane).  On the host the statement is inert.
template <class Ptr>
__device__ __forceinline__ Ptr scalar_base(Ptr p) {
    asm volatile("" : "+s"(p));
    return p;
}

// ------------------------------------------------------------------------------------------------
// The kernel: a persistent grid, FFT f = blockIdx.x, blockIdx.x + gridDim.x, ... < nFFTs.
// amdgpu_waves_per_eu(4): at most 128 VGPRs, so that 16 waves (one 16384 or two 8192 workgroups) fit a CU.
// ------------------------------------------------------------------------------------------------
template <int N, int DIR>
__global__ __launch_bounds__(N / 16) __attribute__((amdgpu_waves_per_eu(4))) void large_c2c(const float2* d_input, float2* d_output, int nFFTs) {
    using G = LargeGeometry<N>;
    __shared__ float2 lds[G::kLdsFloat2];
    LargeEngine<N, DIR> e(threadIdx.x);
    long f = blockIdx.x;
    if (f >= nFFTs) return;
    float2 r[16], y[16];
    for (;;) {
        const long next = f + gridDim.x;
        e.reload_twiddles();
        e.load(r, d_input + f * N);
        large_transform<N, DIR>(e, r, y, lds);      // its last barrier frees the image for the next FFT's exchange A
        e.store(y, d_output + f * N);
        if (next >= nFFTs) break;
        f = next;
    }
}

}  // namespace large
}  // namespace smfft

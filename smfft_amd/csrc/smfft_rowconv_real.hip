// smfft_rowconv_real.hip -- libsmfft_rowconv_real.so: batched linear convolution or correlation of pairs of REAL rows, a[r] with b[r]
// (n_a + n_b - 1 <= 4096), on the register engine's transforms of M = 256 ... 4096 points, in one kernel and one pass through HBM, and
// the C ABI of include/smfft_rowconv_real.h.
//
// Compiled once per M (Makefile: -DSMFFT_ROWCONV_REAL_N=256 ... 4096, flags of their own: ROWCONV_REAL_FLAGS_<M>) for the kernel and its
// launcher, and once without SMFFT_ROWCONV_REAL_N for the C ABI, which checks and dispatches.
//
// rowconv_real_kernel<M> keeps the geometry of rowconv_kernel<M> (smfft_rowconv.hip: 256 threads, 4096 / M rows per workgroup, element
// u + T q in register q, clamped loads and selects, all loads up front behind a scheduling barrier) and runs TWO transforms per pair
// where that kernel runs three: row a goes into the real lane and the second operand into the imaginary lane of one forward transform,
// z = a + i b'; with the partner P[k] = Z[(M - k) mod M], S = Z + conj(P) = 2 A and D = Z - conj(P) = 2 i B, so the spectrum of the
// result is C = A B = S D (-i / 4), and the real part of one inverse transform of C is the answer.
//
// Two unrelated rows in one fp32 number system: the smaller one would drown in the larger one's rounding error.  So each lane is scaled
// by a power of two chosen from that row's own energy (smfft_rowconv_real_scale.hpp: the energy of ldexp(x, k) lies in [1, 4)), and the
// two exponents come off the result with one ldexp.  Every scale is an exact power of two, so scaling a row by 2^s scales its
// results by 2^s to the bit.  The reductions behind the rule -- the largest magnitude, exact, and the fp32 sum of the squares of the row
// scaled by that magnitude's exponent -- run over a thread's sixteen elements in register order, then as an XOR butterfly over the
// lanes that hold the row (every lane ends with the same bits, since a + b is b + a), then, where a row spans two or four waves, over
// the waves' partial results in wave order through sixteen words of LDS with one barrier.  That order depends on nothing but the
// thread layout of a row, which is the same in every slot, tile and grid: the bits of a row's outputs depend on that row pair alone.
//
// The partner comes through the row's LDS region at every M (the registers written in natural order, one fft_sync, sixteen reads: the
// form of HermitianRegisters::kFromLds, smfft_kernels.hpp); where one wave holds the row (M <= 1024) -DSMFFT_ROWCONV_REAL_SPLIT=1 builds
// it from thirty-two ds_bpermute instead, without LDS memory and without the two fences (tools/ab_rowconv_real.py times the two).
//
// The row loads and stores are 4-byte accesses with the engine's policy (gload / gstore: non-temporal); -DSMFFT_NT=0 (make
// EXTRA_HIPFLAGS=-DSMFFT_NT=0 ROWCONV_REAL_LIB=... ROWCONV_REAL_OBJDIR=...) builds them plain for the A/B of tools/ab_rowconv_real.py.
// -DSMFFT_TIMING_ONLY_ROWCONV_REAL_NO_BALANCE=1 leaves the reductions and the scaling out, for that tool's measurement of their cost:
// such a build loses digits where the rows' energies differ and does not keep zero and NaN rows apart; it is never shipped.
#include <hip/hip_runtime.h>

#include "smfft_rowconv_real.h"

namespace smfft {
namespace rowconv_real {
// enqueue `grid` workgroups on `stream`; 0 or the launch's hipError_t.  Defined per M by the objects compiled with -DSMFFT_ROWCONV_REAL_N.
template <int M>
int launch_rows(const float* a, const float* b, float* out, int n_a, int n_b, int first, int m, long long batch, int correlate, int grid, hipStream_t stream);
}  // namespace rowconv_real
}  // namespace smfft

#ifdef SMFFT_ROWCONV_REAL_N
#include "smfft_fir_kernel.hpp"
#include "smfft_rowconv_real_scale.hpp"

// where the partner Z[M - k] comes from: 0 = the row's LDS region (every M), 1 = ds_bpermute where one wave holds the row (M <= 1024)
#ifndef SMFFT_ROWCONV_REAL_SPLIT
#define SMFFT_ROWCONV_REAL_SPLIT 0
#endif
#ifndef SMFFT_TIMING_ONLY_ROWCONV_REAL_NO_BALANCE
#define SMFFT_TIMING_ONLY_ROWCONV_REAL_NO_BALANCE 0
#endif

namespace smfft {
namespace rowconv_real {

// one float with the policy of the engine's gload / gstore
__device__ __forceinline__ float gload1(const float* p) {
#if SMFFT_NT
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}
__device__ __forceinline__ void gstore1(float* p, float v) {
#if SMFFT_NT
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}

// the reductions of one row over the LANES lanes that hold it inside a wave: an XOR butterfly, after which every lane has the same bits
template <int LANES>
__device__ __forceinline__ unsigned lanes_max(unsigned v) {
#pragma unroll
    for (int d = 1; d < LANES; d *= 2) {
        const unsigned o = (unsigned)__shfl_xor((int)v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}
template <int LANES>
__device__ __forceinline__ float lanes_sum(float v) {
#pragma unroll
    for (int d = 1; d < LANES; d *= 2) v += __shfl_xor(v, d, 64);
    return v;
}

// sum_q ldexp(x[q], -p)^2 in register order
__device__ __forceinline__ float squares(const float (&x)[16], int p) {
    float acc = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const float v = ldexpf(x[q], -p);
        acc = __builtin_fmaf(v, v, acc);
    }
    return acc;
}

// out[r m + i] = Re IDFT_M(C)[first + i], i < m, C = A B / M from Z = DFT_M(pad_M(2^ka a[r n_a + .]) + i pad_M(2^kb b'[r])), scaled back
// by 2^-(ka + kb), with b'[e] = b[r n_b + e] (convolve) or b[r n_b + n_b - 1 - e] (correlate), e < n_b.  a and b may be the same buffer:
// no __restrict__ on them.
template <int M>
__global__ void __launch_bounds__(kFirThreads) rowconv_real_kernel(const float* a, const float* b, float* out, int n_a, int n_b, int first, int m, long long batch,
                                                                   int correlate) {
    using G = Geometry<M>;
    constexpr int T = G::T;
    constexpr int kRowLanes = T < 64 ? T : 64;              // lanes of one wave that hold a row
    constexpr int kRowWaves = T / kRowLanes;                // waves that hold a row: 1, or 2 and 4 at M = 2048 and 4096
    constexpr bool kBalance = SMFFT_TIMING_ONLY_ROWCONV_REAL_NO_BALANCE == 0;
    constexpr bool kPartnerOnLanes = SMFFT_ROWCONV_REAL_SPLIT != 0 && !G::kMultiWave;
    __shared__ float2 s[G::kFftsPerBlock * G::SF];
    __shared__ unsigned red[G::kMultiWave ? 16 : 1];        // per wave: max |a|, max |b|, the two sums of squares (as bits)
    Engine<M, 0, 1> fwd;
    Engine<M, 1, 1> inv;
    fwd.init(threadIdx.x);
    inv.init(threadIdx.x);
    float2* sf = s + fwd.fft * G::SF;
    const long long ntiles = (batch + G::kFftsPerBlock - 1) / G::kFftsPerBlock;
    // S D (-i / 4) / M: the inverse transform is un-normalised.  An exact power of two.
    const float scale = 0.25f / (float)M;
    // element e of the second operand is b[bfirst + bstep e]: b[e], or b[n_b - 1 - e]
    const int bfirst = correlate ? n_b - 1 : 0, bstep = correlate ? -1 : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // Z[M - (u + T q)] is register 15 - q of thread (T - u) mod T; thread 0 pairs with itself, register (16 - q) & 15
    const bool self = fwd.u == 0;
    const int partner_addr = 4 * ((lane - fwd.u) + ((T - fwd.u) % T));
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long g = tile * G::kFftsPerBlock + fwd.fft;
        const bool active = g < batch;
        // a[r n_a + j], zero at j >= n_a, and element e of the second operand, zero at e >= n_b: a clamped in-range address and a select
        // afterwards, so the loads go out back to back; an inactive slot of the last tile reads row 0 and stores nothing
        const float* ar = a + (active ? g : 0) * n_a;
        const float* br = b + (active ? g : 0) * n_b;
        float xa[16], xb[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int j = fwd.u + T * q;
            const int jc = j < n_a ? j : n_a - 1;
            const float v = gload1(ar + jc);
            xa[q] = (j == jc) ? v : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = fwd.u + T * q;
            const int ec = e < n_b ? e : n_b - 1;
            const float v = gload1(br + (bfirst + bstep * ec));
            xb[q] = (e == ec) ? v : 0.f;
        }
        // nothing is scheduled across this point: the 32 loads all go out before the first reduction step
        __builtin_amdgcn_sched_barrier(0);
        int ka = 0, kb = 0;
        bool zero = false, finite = true;
        if constexpr (kBalance) {
            unsigned ma = 0u, mb = 0u;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const unsigned va = __float_as_uint(xa[q]) & kAbsMask, vb = __float_as_uint(xb[q]) & kAbsMask;
                ma = va > ma ? va : ma;
                mb = vb > mb ? vb : mb;
            }
            ma = lanes_max<kRowLanes>(ma);
            mb = lanes_max<kRowLanes>(mb);
            int pa = max_exponent(ma), pb = max_exponent(mb);
            float sa = lanes_sum<kRowLanes>(squares(xa, pa)), sb = lanes_sum<kRowLanes>(squares(xb, pb));
            if constexpr (kRowWaves > 1) {
                // a wave's sum is scaled by its own wave's exponent; the row's takes them in wave order, each moved to the row's exponent
                // by an exact power of two.  (The words' previous readers are more than one barrier back: the transforms have several.)
                if (lane == 0) {
                    red[4 * wave + 0] = ma;
                    red[4 * wave + 1] = mb;
                    red[4 * wave + 2] = __float_as_uint(sa);
                    red[4 * wave + 3] = __float_as_uint(sb);
                }
                __syncthreads();
                const unsigned* part = red + 4 * kRowWaves * fwd.fft;
                unsigned wa[kRowWaves], wb[kRowWaves];
                ma = 0u, mb = 0u;
#pragma unroll
                for (int w = 0; w < kRowWaves; ++w) {
                    wa[w] = part[4 * w + 0];
                    wb[w] = part[4 * w + 1];
                    ma = wa[w] > ma ? wa[w] : ma;
                    mb = wb[w] > mb ? wb[w] : mb;
                }
                pa = max_exponent(ma), pb = max_exponent(mb);
                sa = 0.f, sb = 0.f;
#pragma unroll
                for (int w = 0; w < kRowWaves; ++w) {
                    sa += ldexpf(__uint_as_float(part[4 * w + 2]), 2 * (max_exponent(wa[w]) - pa));
                    sb += ldexpf(__uint_as_float(part[4 * w + 3]), 2 * (max_exponent(wb[w]) - pb));
                }
            }
            const RowScale ra = row_scale(ma, __float_as_uint(sa)), rb = row_scale(mb, __float_as_uint(sb));
            ka = ra.k, kb = rb.k;
            zero = (ra.zero | rb.zero) != 0;
            finite = (ra.finite & rb.finite) != 0;
        }
        float2 r[16], p[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) r[q] = kBalance ? make_float2(ldexpf(xa[q], ka), ldexpf(xb[q], kb)) : make_float2(xa[q], xb[q]);
        fft_sync<G::kMultiWave>();             // the previous tile's inverse transform is done with the region
        fwd.transform(r, sf);
        if constexpr (kPartnerOnLanes) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float2 src = r[15 - q];
                const float px = __int_as_float(__builtin_amdgcn_ds_bpermute(partner_addr, __float_as_int(src.x)));
                const float py = __int_as_float(__builtin_amdgcn_ds_bpermute(partner_addr, __float_as_int(src.y)));
                p[q] = self ? r[(16 - q) & 15] : make_float2(px, py);
            }
        } else {
            fft_sync<G::kMultiWave>();         // the transform's last LDS reads are done
#pragma unroll
            for (int q = 0; q < 16; ++q) sf[fwd.u + T * q] = r[q];
            fft_sync<G::kMultiWave>();
            // Z[M - (u + T q)] = Z[(T - u) + T (15 - q)]; thread 0's q = 0 reads one element past the data, inside the region's
            // padding, and takes its own Z[0] instead
            const float2* partner = sf + (T - fwd.u);
#pragma unroll
            for (int q = 0; q < 16; ++q) p[q] = partner[T * (15 - q)];
            p[0] = self ? r[0] : p[0];
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float2 S = make_float2(r[q].x + p[q].x, r[q].y - p[q].y);       // Z + conj(P) = 2 A
            const float2 D = make_float2(r[q].x - p[q].x, r[q].y + p[q].y);       // Z - conj(P) = 2 i B
            // S D (-i) = (Im(S D), -Re(S D)), each one rounded product and one fused multiply-add
            const float im = __builtin_fmaf(S.x, D.y, S.y * D.x), re = __builtin_fmaf(S.x, D.x, -(S.y * D.y));
            r[q] = make_float2(im * scale, -re * scale);
        }
        fft_sync<G::kMultiWave>();             // the partner reads (or the forward transform's last LDS reads) are done
        inv.transform(r, sf);
        float* yr = out + g * m;
        const unsigned mend = active ? (unsigned)m : 0u;
        const int back = -(ka + kb);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int i = fwd.u + T * q - first;         // element k = first + i of the row's full result goes to yr[i], 0 <= i < m
            float y = kBalance ? ldexpf(r[q].x, back) : r[q].x;
            // a pair with a row of zeros stores +0 -- times 0 plus +0, so that a NaN of the partner stays one -- and a pair with an Inf
            // or a NaN stores NaN in every element, whatever the transforms made of it
            y = zero ? __builtin_fmaf(y, 0.f, 0.f) : y + 0.f;
            y = finite ? y : __builtin_nanf("");
            if ((unsigned)i < mend) gstore1(yr + i, y);
        }
    }
}

template <>
int launch_rows<SMFFT_ROWCONV_REAL_N>(const float* a, const float* b, float* out, int n_a, int n_b, int first, int m, long long batch, int correlate, int grid,
                                      hipStream_t stream) {
    hipLaunchKernelGGL(rowconv_real_kernel<SMFFT_ROWCONV_REAL_N>, dim3((unsigned)grid), dim3(kFirThreads), 0, stream, a, b, out, n_a, n_b, first, m, batch, correlate);
    return (int)hipGetLastError();
}

}  // namespace rowconv_real
}  // namespace smfft

#else  // the C ABI
#include "smfft_rows_host.hpp"

namespace {
constexpr int kMaxFull = 4096;      // the largest n_a + n_b - 1

// M: the smallest of 256 ... 4096 with M >= n_a + n_b - 1; -1 outside the range (the sum is taken in 64 bits: no overflow at INT_MAX)
int fft_size(int n_a, int n_b) {
    if (n_a < 1 || n_b < 1 || (long long)n_a + n_b - 1 > kMaxFull) return -1;
    int M = 256;
    while (M < n_a + n_b - 1) M *= 2;
    return M;
}

// the launch of `grid` workgroups (<= 0: the default) on `stream`
auto dispatch(const void* a, const void* b, void* out, int n_a, int n_b, int first, int m, long long batch, int correlate) {
    return [=](int grid, hipStream_t stream) {
        const int M = fft_size(n_a, n_b);
        grid = default_grid(M, batch, grid);
        return dispatch_m(M, [&](auto len) {
            return smfft::rowconv_real::launch_rows<len()>((const float*)a, (const float*)b, (float*)out, n_a, n_b, first, m, batch, correlate != 0, grid, stream);
        });
    };
}

// -1: refused; 0: launch; 1: nothing to do.  No HIP call.  The window lies inside the full result (first + m in 64 bits); the output is
// neither input, whatever the batch.
int check(const void* a, const void* b, const void* out, int n_a, int n_b, int first, int m, long long batch) {
    if (fft_size(n_a, n_b) < 0 || first < 0 || m < 1 || (long long)first + m > (long long)n_a + n_b - 1) return -1;
    if (batch < 0 || out == a || out == b) return -1;
    return batch == 0 ? 1 : 0;
}
}  // namespace

extern "C" {

int smfft_rowconv_real_fft_size(int n_a, int n_b) { return fft_size(n_a, n_b); }

int smfft_rowconv_real_launch(const void* d_a, const void* d_b, void* d_out, int n_a, int n_b, int first, int m, long long batch, int correlate, void* hip_stream) {
    return checked_launch(check(d_a, d_b, d_out, n_a, n_b, first, m, batch), dispatch(d_a, d_b, d_out, n_a, n_b, first, m, batch, correlate), hip_stream);
}

int smfft_rowconv_real_launch_tuned(const void* d_a, const void* d_b, void* d_out, int n_a, int n_b, int first, int m, long long batch, int correlate, void* hip_stream,
                                    int grid) {
    return checked_launch_tuned(check(d_a, d_b, d_out, n_a, n_b, first, m, batch), dispatch(d_a, d_b, d_out, n_a, n_b, first, m, batch, correlate), hip_stream, grid);
}

int smfft_rowconv_real_benchmark(const void* d_a, const void* d_b, void* d_out, int n_a, int n_b, int first, int m, long long batch, int correlate, double* FFT_time) {
    return checked_benchmark(check(d_a, d_b, d_out, n_a, n_b, first, m, batch), dispatch(d_a, d_b, d_out, n_a, n_b, first, m, batch, correlate), FFT_time);
}

}  // extern "C"
#endif

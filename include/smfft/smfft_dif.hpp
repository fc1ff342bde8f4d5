// smfft_dif.hpp -- decimation-in-frequency (DIF) C2C transforms in the reference's contract: natural order in, BIT-REVERSED
// spectrum out.
//
//   do_SMFFT_CT_DIF<P>(s)                       s[j] = X[bitrev(j)] in place; blockDim.x = fft_length / 4, as do_SMFFT_CT_DIT<P>
//   do_SMFFT_CT_DIF_registers<P>(x, s_scratch)  N >= 256, one transform per block of N / 4 threads: x[m] = element t + m N/4 in,
//                                               x[m] = position 4 t + m of the bit-reversed result out
//
// P is one of the FFT_<N>_{forward,inverse}_noreorder classes (the _wave64 classes of N = 32 / 64 / 128 included); X is the
// un-normalised DFT with P's sign.  The transform is the TRANSPOSE of the no-reorder DIT ladder of the same class: the passes in
// reverse order, the twiddles after the butterfly.  So the no-reorder DIT transform of the other sign is its exact inverse partner,
// DIT_noreorder_inverse(DIF_forward(x)) = N x, and a circular convolution needs no reordering at all:
//     DIT_noreorder_inverse(DIF_forward(x) . DIF_forward(h)) = N (x (*) h)
// (the filter goes through the same DIF transform once).  The output of do_SMFFT_CT_DIF_registers is the
// input of do_SMFFT_CT_DIT_registers<FFT_<N>_*_noreorder> as it stands ("element 4 threadIdx.x + m"), and the two need no workgroup
// barrier between them (below).
//
// Ladder (radix-2 Gentleman-Sande stages, two fused per pass; tools/dif_ladder_model.py replays it against numpy.fft):
//   odd log2 N:  a radix-2 pass first on x[t + m N/4]: (e0, e2) <- (e0 + e2, (e0 - e2) W_N^t), (e1, e3) likewise with -+i W_N^t
//   pass L (quarter span L = N/4 or N/8, then / 4 down to 1): thread t holds elements a + m L, a = (t / L) 4L + k, k = t mod L:
//        s0 = e0 + e2, d0 = e0 - e2, s1 = e1 + e3, d1 = -+i (e1 - e3)
//        e0 <- s0 + s1,  e1 <- (s0 - s1) w1,  e2 <- (d0 + d1) w2,  e3 <- (d0 - d1) w3      w2 = W_4L^k, w1 = w2^2, w3 = w1 w2
//   -- the twiddles of the DIT ladder's pass P = L (QuarterTwiddleRows: same rows, one load per thread and pass, fetched in front of the
//   first synchronisation).  The first pass consumes the natural-order coalesced load; the last (L = 1, no twiddles) leaves a thread
//   the four bit-reversed positions 4 t + m: the bit reversal costs nothing, neither a trip through LDS nor a scattered store.
// Between passes the data go through the swizzled image of the DIT ladder (quarter_swizzle: a thread's accesses of a pass are the
// DIT ladder's of the same span, so the model counts every read conflict free and the stores at most 2-way).
// Synchronisation: the elements of a pass with L <= 64 lie in the aligned block of 256 of the thread's wave (t / L groups of 4L with
// L | 64), and the swizzle permutes aligned groups of 32 -- a wave-level fence orders them.  Only the writes of the radix-2 pass and of
// the passes with L >= 256 are read by other waves: N = 512 / 1024 one workgroup barrier, N = 2048 / 4096 two (N <= 256: none).  The
// LAST pass reads the wave's own block only, so a DIT-noreorder transform that starts on the same wave's block (its first four passes
// and their exchange, smfft_device_functions.hpp quarter_fft kLanesHead) needs no barrier behind it -- at every length.
// Contract form: the first pass reads s in natural order and the first image store follows a synchronisation (a barrier for
// N >= 512); the last pass stores its four positions 4 t + m in natural layout behind a wave-level fence.
#pragma once
#include "smfft_device_functions.hpp"

namespace smfft {

template <int N>
struct DifPlan {
    static constexpr int kBits = ilog2c(N);
    static constexpr bool kOdd = (kBits & 1) != 0;
    static constexpr int kQuads = kBits / 2;                          // fused passes, quarter spans 4^(kQuads-1) ... 1
    static constexpr int kPasses = kQuads + (kOdd ? 1 : 0);           // pass 0 is the radix-2 pass of an odd log2 N
    static constexpr bool radix2(int j) { return kOdd && j == 0; }
    __host__ __device__ static constexpr int span(int j) { return 1 << (2 * (kQuads - 1 - (j - (kOdd ? 1 : 0)))); }
    // element m of thread t (index within the transform) in pass j -- what it reads and where its results go
    __host__ __device__ static constexpr int element(int j, int t, int m) {
        return radix2(j) ? t + m * (N / 4) : ((t / span(j)) * 4 * span(j)) + (t % span(j)) + m * span(j);
    }
    // the pass's results are read by other waves (its elements are not inside the thread's aligned block of 256)
    static constexpr bool crosses_waves(int j) { return N > 256 && (radix2(j) || span(j) >= 256); }
    // index into twiddle_values of w2 (W_4L^k) / of W_N^t for the radix-2 pass; -1: no twiddle (L = 1)
    __host__ __device__ static constexpr int twiddle_index(int j, int t) {
        return radix2(j) ? (t * (4096 / N)) & 4095 : span(j) == 1 ? -1 : ((t % span(j)) * (4096 / (4 * span(j)))) & 4095;
    }
    // ... its place in the rows of QuarterTwiddleRows<N> (row p >= 1 holds W_4P^k, P = 4^p; the radix-2 row W_N^t after them)
    __host__ __device__ static constexpr int twiddle_row_entry(int j, int t) {
        return radix2(j) ? QuarterTwiddleRows<N>::row_start(QuarterTwiddleRows<N>::kPasses) + t
                         : QuarterTwiddleRows<N>::row_start(ilog2c(span(j)) / 2) + t % span(j);
    }
};

// (-+i) v: the forward transform's W_4 = -i
template <int DIR>
__device__ __forceinline__ float2 dif_mul_mi(float2 v) { return DIR ? make_float2(-v.y, v.x) : make_float2(v.y, -v.x); }

template <int DIR>
__device__ __forceinline__ void dif_quad_butterfly(float2 (&e)[4], float2 w2, bool trivial) {
    const float2 s0 = cadd(e[0], e[2]), d0 = csub(e[0], e[2]), s1 = cadd(e[1], e[3]);
    const float2 d1 = dif_mul_mi<DIR>(csub(e[1], e[3]));
    e[0] = cadd(s0, s1);
    if (trivial) {
        e[1] = csub(s0, s1), e[2] = cadd(d0, d1), e[3] = csub(d0, d1);
    } else {
        const float2 w1 = make_float2(w2.x * w2.x - w2.y * w2.y, 2.f * w2.x * w2.y);
        e[1] = cmul(csub(s0, s1), w1), e[2] = cmul(cadd(d0, d1), w2), e[3] = cmul(csub(d0, d1), cmul(w1, w2));
    }
}

// BLOCK_THREADS: threads of ONE transform's share of the block that must synchronise (> 64: a workgroup barrier where data cross
// waves); s: the block's LDS (the image uses s[region_offset .. + N)); t: the thread's index in its transform.
// IN_REGS: x[m] = element t + m N/4 going in (s need only be free); otherwise s[region_offset + n] holds the input in natural order.
// OUT_REGS: x[m] = position 4 t + m of the result coming out; otherwise it is stored there in s (natural layout).
template <int N, int DIR, int BLOCK_THREADS, bool IN_REGS, bool OUT_REGS>
__device__ __forceinline__ void dif_ladder(float2 (&x)[4], float2* s, int t, int region_offset) {
    using D = DifPlan<N>;
    constexpr bool kMulti = BLOCK_THREADS > 64;
    // the twiddles first: they depend on the thread only (w[j] = w2 of pass j)
    float2 w[D::kPasses];
#pragma unroll
    for (int j = 0; j < D::kPasses; ++j) {
        w[j] = make_float2(1.f, 0.f);
        if (D::radix2(j) || D::span(j) > 1) {
            const TwiddleValue tv = quarter_twiddle_rows<N>.w[D::twiddle_row_entry(j, t)];
            w[j] = make_float2(tv.x, DIR ? -tv.y : tv.y);
        }
    }
    float2 e[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) e[m] = IN_REGS ? x[m] : s[region_offset + t + m * (N / 4)];
    if constexpr (!IN_REGS) fft_sync<kMulti>();              // every natural-order read precedes the stores into the image
#pragma unroll
    for (int j = 0; j < D::kPasses; ++j) {
        if (j > 0) {
#pragma unroll
            for (int m = 0; m < 4; ++m) e[m] = s[quarter_swizzle(region_offset + D::element(j, t, m))];
        }
        if (D::radix2(j)) {
            const float2 a0 = cadd(e[0], e[2]), a1 = cadd(e[1], e[3]);
            const float2 b0 = cmul(csub(e[0], e[2]), w[j]), b1 = cmul(csub(e[1], e[3]), w[j]);
            e[0] = a0, e[1] = a1, e[2] = b0, e[3] = dif_mul_mi<DIR>(b1);
        } else {
            dif_quad_butterfly<DIR>(e, w[j], D::span(j) == 1);
        }
        if (j + 1 < D::kPasses) {
#pragma unroll
            for (int m = 0; m < 4; ++m) s[quarter_swizzle(region_offset + D::element(j, t, m))] = e[m];
            if (D::crosses_waves(j) && kMulti) fft_sync<true>();
            else fft_sync<false>();
        }
    }
    // the last pass read the wave's own aligned block only: a wave-level fence orders those reads before any later store into it
    // (the natural-layout stores below, or the caller's next transform)
    fft_sync<false>();
    if constexpr (OUT_REGS) {
#pragma unroll
        for (int m = 0; m < 4; ++m) x[m] = e[m];
    } else {
#pragma unroll
        for (int m = 0; m < 4; ++m) s[region_offset + 4 * t + m] = e[m];
    }
}

}  // namespace smfft

// =================================================================================================
// the reference's contract
// =================================================================================================
template <class const_params>
__device__ void do_SMFFT_CT_DIF(float2* s_input) {
    static_assert(const_params::fft_reorder == 0, "the DIF transform is the transpose of a no-reorder (FFT_<N>_*_noreorder) class");
    constexpr int N = const_params::fft_size;
    constexpr int kBlock = const_params::fft_length / 4;                 // 32 threads hold 128 / N transforms for N <= 128 (CT:586-595)
    const int f = threadIdx.x / (N / 4), t = threadIdx.x % (N / 4);
    float2 x[4];
    smfft::dif_ladder<N, const_params::fft_direction, kBlock, false, false>(x, s_input, t, f * N);
}

template <class const_params>
__device__ void do_SMFFT_CT_DIF_registers(float2 (&x)[4], float2* s_scratch) {
    static_assert(const_params::fft_reorder == 0, "the DIF transform is the transpose of a no-reorder (FFT_<N>_*_noreorder) class");
    constexpr int N = const_params::fft_size;
    static_assert(N >= 256 && const_params::fft_length == N, "one transform per block of N / 4 threads");
    smfft::dif_ladder<N, const_params::fft_direction, N / 4, true, true>(x, s_scratch, threadIdx.x, 0);
}

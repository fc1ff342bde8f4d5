// smfft_rowconv.hip -- libsmfft_rowconv.so: batched linear convolution or correlation of pairs of complex rows, a[r] with b[r]
// (n_a + n_b - 1 <= 4096), on the register engine's transforms of M = 256 ... 4096 points, in one kernel and one pass through HBM, and
// the C ABI of include/smfft_rowconv.h.
//
// Compiled once per M (Makefile: -DSMFFT_ROWCONV_N=256 ... 4096, flags of their own: ROWCONV_FLAGS_<M>) for the kernel and its
// launcher, and once without SMFFT_ROWCONV_N for the C ABI, which checks and dispatches.
//
// rowconv_kernel<M> is the chain of the FIR, Bluestein and chirp-z kernels (DESIGN.md sections 16, 18 and 19) with the prepared spectrum
// replaced by a second forward transform of data: a thread loads all sixteen elements u + T q of its row of a and of the second
// operand, since either of n_a, n_b may exceed M / 2, transforms both, multiplies, transforms back and stores the elements of the
// window.  There are no tables: a thread carries two row buffers of sixteen float2 where the chirp-z kernel carries one and 32 to 48
// table elements.  Both rows' 32 loads are issued up front, back to back, in front of the first transform, and a scheduling barrier
// behind them keeps the compiler from sinking b's loads and the selects into the transform: 194 ... 249 registers, two waves per SIMD at
// every M, as with b loaded behind the first transform (175 ... 236), which would leave half as many loads in flight; without the
// scheduling barrier the up-front form came to 252 and 260 registers at M = 2048 and 4096 (DESIGN.md section 20 has the figures of all
// three).  The body is written out in the kernel itself, for the reason smfft_fir_kernel.hpp gives.
//
// The row loads and stores are the engine's gload / gstore: non-temporal, as in the FIR banks.  -DSMFFT_NT=0 (make
// EXTRA_HIPFLAGS=-DSMFFT_NT=0 ROWCONV_LIB=... ROWCONV_OBJDIR=...) builds them plain for the A/B of tools/ab_rowconv.py (DESIGN.md
// section 20).  -DSMFFT_ROWCONV_LATE_B=1 builds b's loads behind the first transform, for the same tool.
#include <hip/hip_runtime.h>

#include "smfft_rowconv.h"

namespace smfft {
namespace rowconv {
// enqueue `grid` workgroups on `stream`; 0 or the launch's hipError_t.  Defined per M by the objects compiled with -DSMFFT_ROWCONV_N.
template <int M>
int launch_rows(const float2* a, const float2* b, float2* out, int n_a, int n_b, int first, int m, long long batch, int correlate, int grid, hipStream_t stream);
}  // namespace rowconv
}  // namespace smfft

#ifdef SMFFT_ROWCONV_N
#include "smfft_fir_kernel.hpp"

// where b's loads are issued: 0 = up front, behind a's (ships); 1 = behind the first transform
#ifndef SMFFT_ROWCONV_LATE_B
#define SMFFT_ROWCONV_LATE_B 0
#endif

namespace smfft {
namespace rowconv {

// out[r m + i] = IDFT_M(DFT_M(pad_M(a[r n_a + .])) DFT_M(pad_M(b'[r] / M)))[first + i], i < m, with b'[e] = b[r n_b + e] (convolve) or
// conj(b[r n_b + n_b - 1 - e]) (correlate), e < n_b.  a and b may be the same buffer: no __restrict__ on them.
template <int M>
__global__ void __launch_bounds__(kFirThreads) rowconv_kernel(const float2* a, const float2* b, float2* out, int n_a, int n_b, int first, int m, long long batch,
                                                              int correlate) {
    using G = Geometry<M>;
    constexpr bool kLateB = SMFFT_ROWCONV_LATE_B != 0;
    __shared__ float2 s[G::kFftsPerBlock * G::SF];
    Engine<M, 0, 1> fwd;
    Engine<M, 1, 1> inv;
    fwd.init(threadIdx.x);
    inv.init(threadIdx.x);
    float2* sf = s + fwd.fft * G::SF;
    const long long ntiles = (batch + G::kFftsPerBlock - 1) / G::kFftsPerBlock;
    // 1 / M, an exact power of two, goes onto the second operand at its load: no prepared spectrum exists that could carry it.  The
    // imaginary part takes the sign of the conjugate with it.
    const float scale = 1.0f / (float)M;
    const float iscale = correlate ? -scale : scale;
    // element e of the second operand is b[bfirst + bstep e]: b[e], or b[n_b - 1 - e] under the conjugate
    const int bfirst = correlate ? n_b - 1 : 0, bstep = correlate ? -1 : 1;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long g = tile * G::kFftsPerBlock + fwd.fft;
        const bool active = g < batch;
        // a[r n_a + j], zero at j >= n_a, and element e of the second operand, zero at e >= n_b: a clamped in-range address and a select
        // afterwards, so the loads go out back to back; an inactive slot of the last tile reads row 0 and stores nothing
        const float2* ar = a + (active ? g : 0) * n_a;
        const float2* br = b + (active ? g : 0) * n_b;
        float2 r[16], p[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int j = fwd.u + G::T * q;
            const int jc = j < n_a ? j : n_a - 1;
            const float2 v = gload(ar + jc);
            r[q] = (j == jc) ? v : make_float2(0.f, 0.f);
        }
        if constexpr (kLateB) {
            __builtin_amdgcn_sched_barrier(0);
            fft_sync<G::kMultiWave>();         // the previous tile's inverse transform is done with the region
            fwd.transform(r, sf);
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = fwd.u + G::T * q;
            const int ec = e < n_b ? e : n_b - 1;
            const float2 v = gload(br + (bfirst + bstep * ec));
            const float2 w = (e == ec) ? v : make_float2(0.f, 0.f);
            p[q] = make_float2(w.x * scale, w.y * iscale);
        }
        // nothing is scheduled across this point: the loads above all go out before the first butterfly, and the compiler neither sinks
        // b's loads into the transform nor waits for a's one by one to apply their selects early (it did both: DESIGN.md section 20)
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (!kLateB) {
            fft_sync<G::kMultiWave>();         // the previous tile's inverse transform is done with the region
            fwd.transform(r, sf);
        }
        fft_sync<G::kMultiWave>();             // the first transform's last LDS reads are done
        fwd.transform(p, sf);
#pragma unroll
        for (int q = 0; q < 16; ++q) r[q] = cmul_fixed(r[q], p[q]);
        fft_sync<G::kMultiWave>();             // the second transform's last LDS reads are done
        inv.transform(r, sf);
        float2* yr = out + g * m;
        const unsigned mend = active ? (unsigned)m : 0u;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int i = fwd.u + G::T * q - first;      // element k = first + i of the row's full result goes to yr[i], 0 <= i < m
            // + 0: the conjugate of a zero is -0, and a pair with a row of zeros stores +0 in every element
            if ((unsigned)i < mend) gstore(yr + i, make_float2(r[q].x + 0.f, r[q].y + 0.f));
        }
    }
}

template <>
int launch_rows<SMFFT_ROWCONV_N>(const float2* a, const float2* b, float2* out, int n_a, int n_b, int first, int m, long long batch, int correlate, int grid,
                                 hipStream_t stream) {
    hipLaunchKernelGGL(rowconv_kernel<SMFFT_ROWCONV_N>, dim3((unsigned)grid), dim3(kFirThreads), 0, stream, a, b, out, n_a, n_b, first, m, batch, correlate);
    return (int)hipGetLastError();
}

}  // namespace rowconv
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
            return smfft::rowconv::launch_rows<len()>((const float2*)a, (const float2*)b, (float2*)out, n_a, n_b, first, m, batch, correlate != 0, grid, stream);
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

int smfft_rowconv_fft_size(int n_a, int n_b) { return fft_size(n_a, n_b); }

int smfft_rowconv_launch(const void* d_a, const void* d_b, void* d_out, int n_a, int n_b, int first, int m, long long batch, int correlate, void* hip_stream) {
    return checked_launch(check(d_a, d_b, d_out, n_a, n_b, first, m, batch), dispatch(d_a, d_b, d_out, n_a, n_b, first, m, batch, correlate), hip_stream);
}

int smfft_rowconv_launch_tuned(const void* d_a, const void* d_b, void* d_out, int n_a, int n_b, int first, int m, long long batch, int correlate, void* hip_stream,
                               int grid) {
    return checked_launch_tuned(check(d_a, d_b, d_out, n_a, n_b, first, m, batch), dispatch(d_a, d_b, d_out, n_a, n_b, first, m, batch, correlate), hip_stream, grid);
}

int smfft_rowconv_benchmark(const void* d_a, const void* d_b, void* d_out, int n_a, int n_b, int first, int m, long long batch, int correlate, double* FFT_time) {
    return checked_benchmark(check(d_a, d_b, d_out, n_a, n_b, first, m, batch), dispatch(d_a, d_b, d_out, n_a, n_b, first, m, batch, correlate), FFT_time);
}

}  // extern "C"
#endif

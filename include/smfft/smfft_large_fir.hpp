// smfft_large_fir.hpp -- overlap-save FIR filter banks with segments of N = 8192 and 16384 (gfx950), on the C2C engine of
// smfft_large.hpp: C channels of a long complex signal, each filtered by K filters of up to N - 1 taps, in one kernel from segment
// load to filtered output (include/smfft_large_fir.h; the semantics of the "FIR filter banks" of include/smfft.h).
//
// The engine and its geometry are used as they are.  What makes the fusion cheap is a fact of that engine: pass 1 consumes
// x[u + T*c] and pass 4 produces X[u + T*q] -- the same sixteen positions per thread.  The forward transform's output registers are,
// after a multiplication by H_k[u + T*q] (coalesced loads), exactly the inverse transform's input registers: no exchange between the
// two transforms, no reordering, and the store window is an index test on j = u + T*q.  (tools/large_fir_model.py replays it in fp64.)
//
// One unit of work is done by one workgroup of T = N / 16 threads; the units of a launch are folded into one grid dimension and a
// persistent grid strides over them:
//   * load segment s of channel c: x_c[a(s) + u + T*q], zero outside [0, L).  Sixteen loads from a clamped in-range address with
//     zero selected afterwards, so that they are unconditional and go out back to back;
//   * forward passes 1-4: X[u + T*q] in registers;
//   * for each filter k of the unit: P = X H_k (cmul_fixed: every filter's arithmetic is the same to the bit, whichever unit runs it),
//     inverse passes 1-4, predicated non-temporal store of the elements j in [M - 1, store_end(s)) to out[(c K + k) L + n(s, j)].
// Every output element is written exactly once.  The segmentation is smfft::FirWindow (smfft_fir.hpp), shared with the host.
//
// Two forms of the loop, one source (template parameter HELD):
//   * recompute (HELD = 0): a unit is one (segment, filter) pair, unit = (c S + s) K + k -- one forward and one inverse transform; the
//     K - 1 other units of a segment run at the same time on other CUs and re-read it from cache.  Nothing outlives a transform, so
//     the kernel keeps the C2C kernels' occupancy (at most 128 VGPRs: one 16384 or two 8192 workgroups per CU).
//   * held (HELD = 1, N = 8192 only): a unit is one segment and a group of `group_size` filters, unit = (c S + s) G + g with
//     G = ceil(K / group_size) -- one forward and up to group_size inverse transforms, the spectrum X (32 VGPRs) kept across them.
//     That does not fit 128 VGPRs: one workgroup per CU (amdgpu_waves_per_eu(2)).  At 16384 X cannot be held anywhere on chip.
// The window arithmetic is 32-bit: the 64-bit part is folded into one uniform base pointer per segment (x_c + a(s), and the output
// row + s V - (M - 1)), and the element number e = u + T*q in [0, N) is clamped / tested against two uniform 32-bit bounds.
//
// Barriers: the six of each transform (smfft_large.hpp), twelve per (forward + inverse).  The engine's sixth barrier frees the
// image for the next transform's exchange A, whichever transform that is.
// There is no prefetch of the next segment across iterations.
//
// Buffer contract (include/smfft_large_fir.h): 8-byte-aligned pointers, 64-bit element offsets, only signal[0, C L), spectra[0, K N)
// and out[0, C K L) touched; the three must not overlap.
#pragma once
#include <hip/hip_runtime.h>
#include "smfft_large.hpp"
#include "smfft_fir.hpp"      // smfft::FirWindow, smfft::fir_filter_group_size (smfft_amd/csrc)

namespace smfft {
namespace large {

// The stride of a persistent grid of `grid` workgroups over the units (c S + s) groups + g, in the units' own digits:
// grid = (dc S + ds) groups + dg.  Computed by the host for the launch it makes; the kernel advances (c, s, g) by it.
struct LargeFirStride {
    long long S;       // segments per channel (FirWindow::segments(): a 64-bit division, done once by the host)
    long long dc, ds;
    int dg;
};
__host__ __device__ inline LargeFirStride large_fir_stride(long long grid, int groups, long long S) {
    const long long dcs = grid / groups;
    return LargeFirStride{S, dcs / S, dcs % S, (int)(grid % groups)};
}

// ------------------------------------------------------------------------------------------------
// The filter kernel.  units = C S G (G = K in the recompute form); group_size is 1 in the recompute form; st = large_fir_stride(gridDim.x, G, S).
// ------------------------------------------------------------------------------------------------
template <int N, int HELD>
__global__ __launch_bounds__(N / 16) __attribute__((amdgpu_waves_per_eu(HELD ? 2 : 4)))
void large_fir(const float2* x, const float2* H, float2* y, FirWindow w, int n_filters, int group_size, long long units, LargeFirStride st) {
    static_assert(!HELD || N == 8192, "the spectrum can be held across the filters at N = 8192 only");
    using G = LargeGeometry<N>;
    constexpr int T = G::T;
    __shared__ float2 lds[G::kLdsFloat2];
    LargeEngine<N, 0> fwd(threadIdx.x);
    LargeEngine<N, 1> inv(threadIdx.x);
    const int u = threadIdx.x;
    long long unit = blockIdx.x;
    if (unit >= units) return;
    const long long S = st.S;
    const int groups = HELD ? (n_filters + group_size - 1) / group_size : n_filters;
    const int jbegin = w.store_begin();
    // unit = (c S + s) groups + g.  No 64-bit division here (its expansion keeps these uniform values in vector registers): the
    // workgroup's first unit is its number, which fits 32 bits, and the grid's stride comes decomposed from the host
    // (large_fir_stride) and is added digit by digit with carries
    const long long stride = gridDim.x;
    const unsigned first = blockIdx.x, S32 = S > 0xffffffffll ? 0xffffffffu : (unsigned)S;
    const unsigned cs0 = uniform(first / (unsigned)groups), c0 = uniform(cs0 / S32);
    int g = (int)(first - cs0 * (unsigned)groups);
    long long c = c0, s = cs0 - c0 * S32;
    const long long dc = st.dc, ds = st.ds;
    const int dg = st.dg;
    for (;;) {
        const long long next = unit + stride;
        const int k0 = HELD ? g * group_size : g;
        const int k1 = HELD ? (k0 + group_size < n_filters ? k0 + group_size : n_filters) : k0 + 1;
        // the segment: element e of it is xs[e]; in range for e in [lo, hi), which is never empty (L > s V)
        const long long a = w.load_start(s);
        GlobalFloat2* xs = (GlobalFloat2*)x + uniform(c * w.L + a);
        const int lo = (int)uniform((unsigned)(a < 0 ? (int)-a : 0));
        const int hi = (int)uniform((unsigned)(w.L - a < N ? (int)(w.L - a) : N));
        fwd.reload_twiddles();
        float2 r[16], X[16];
        // every thread loads from a clamped in-range address (a scalar base and a 32-bit lane offset) and zeroes the value afterwards
        // with a bit mask, so that the sixteen loads are unconditional and go out back to back (a select between the loaded value and
        // zero makes hipcc branch around each load)
        unsigned keep[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = u + T * q;
            const int ec = e < lo ? lo : (e < hi ? e : hi - 1);
            keep[q] = e == ec ? 0xffffffffu : 0u;
            r[q] = make_float2(xs[(unsigned)ec].x, xs[(unsigned)ec].y);
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) r[q] = make_float2(__uint_as_float(__float_as_uint(r[q].x) & keep[q]), __uint_as_float(__float_as_uint(r[q].y) & keep[q]));
        large_transform<N, 0>(fwd, r, X, lds);
        const int jend = (int)uniform((unsigned)w.store_end(s));
        // element j of the segment is output row[j] of filter k's row
        float2* row = y + uniform((c * n_filters + k0) * w.L + w.output_index(s, 0));
        GlobalFloat2* Hk = (GlobalFloat2*)H + (long long)k0 * N;      // uniform: the loads are a scalar base and one lane offset
#pragma unroll 1
        for (int k = k0; k < k1; ++k) {
            inv.reload_twiddles();
            float2 h[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                GlobalFloat2* hq = Hk + T * q;      // a scalar base per load, one lane offset for all sixteen
                h[q] = make_float2(hq[(unsigned)u].x, hq[(unsigned)u].y);
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) r[q] = cmul_fixed(X[q], h[q]);
            float2 p[16];
            large_transform<N, 1>(inv, r, p, lds);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int j = u + T * q;
                if (j >= jbegin && j < jend) gstore(row + j, p[q]);
            }
            row += w.L;
            Hk += N;
        }
        if (next >= units) break;
        unit = next;
        g += dg;
        s += ds;
        c += dc;
        if (g >= groups) {
            g -= groups;
            ++s;
        }
        if (s >= S) {
            s -= S;
            ++c;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// H_k = DFT_N(pad_N(g_k)) / N, natural order: g_k = h_k, or g_k[m] = conj(h_k[M - 1 - m]) (correlate).  One workgroup per filter,
// a persistent grid striding over the filters.  The scaling by 1 / N is exact.
// ------------------------------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(N / 16) __attribute__((amdgpu_waves_per_eu(4)))
void large_fir_prepare(const float2* taps, int M, int n_filters, int correlate, float2* spectra) {
    using G = LargeGeometry<N>;
    constexpr int T = G::T;
    __shared__ float2 lds[G::kLdsFloat2];
    LargeEngine<N, 0> fwd(threadIdx.x);
    const int u = threadIdx.x;
    long k = blockIdx.x;
    if (k >= n_filters) return;
    for (;;) {
        const long next = k + gridDim.x;
        const float2* hk = taps + k * M;
        fwd.reload_twiddles();
        float2 r[16], y[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = u + T * q;
            const bool in = e < M;
            const float2 t = hk[in ? (correlate ? M - 1 - e : e) : 0];
            r[q] = in ? make_float2(t.x, correlate ? -t.y : t.y) : make_float2(0.f, 0.f);
        }
        large_transform<N, 0>(fwd, r, y, lds);
#pragma unroll
        for (int q = 0; q < 16; ++q) spectra[k * N + u + T * q] = make_float2(y[q].x * (1.0f / N), y[q].y * (1.0f / N));
        if (next >= n_filters) break;
        k = next;
    }
}

}  // namespace large
}  // namespace smfft

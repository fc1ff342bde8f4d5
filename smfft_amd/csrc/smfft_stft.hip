// smfft_stft.hip -- libsmfft_stft.so: the batched short-time Fourier transform (complex spectrum or power) of real signals in frames of
// n = 512 ... 8192 samples (powers of two) at any hop, and the inverse transform of such frames, on ONE complex transform of
// M = n / 2 = 256 ... 4096 points of the register engine per frame, in one kernel and one pass through HBM, and the C ABI of
// include/smfft_stft.h.
//
// Compiled once per M (Makefile: -DSMFFT_STFT_N=256 ... 4096, flags of their own: STFT_FLAGS_<M>) for the three kernels and their
// launchers, and once without SMFFT_STFT_N for the C ABI, which checks and dispatches.
//
// The geometry is hilbert_kernel's (smfft_hilbert.hip: 256 threads, 4096 / M frames per workgroup, element u + T q in register q,
// workgroups stride over the tiles).  Consecutive pairs of windowed samples are the two lanes of the transform:
// stft_kernel<M, KIND>:
//     z[p] = w[2p] x[2p] + i w[2p+1] x[2p+1]: one 8-byte sample load and one 8-byte window load per element, consecutive lanes at
//            consecutive addresses; the frame is read from the signal itself, in[c stream_stride + f hop ... + n);
//     Z = DFT_M(z); partner P[k] = conj Z[(M - k) mod M] through the row's LDS region (the form of hilbert_kernel);
//     X[k] = (Z[k] + P[k]) / 2 - (i / 2) W_n^k (Z[k] - P[k]), k < M, W_n = exp(-2 pi i / n): the Hermitian split of Z into the spectra of
//            the even and the odd samples and their radix-2 merge.  X[0] = Re Z[0] + Im Z[0] and X[M] = Re Z[0] - Im Z[0], both with an
//            imaginary part of exactly +0, are stored by the thread that owns k = 0.
//     KIND 0 stores the M + 1 complex values (8 bytes per element), KIND 1 re * re + im * im of them (4 bytes per element, consecutive
//            lanes at consecutive floats).
// istft_kernel<M>:
//     A[k] = X[k], B[k] = conj X[M - k] (A[0] = Re X[0], B[0] = Re X[M]: the imaginary parts of the two real bins are ignored) -- the
//            partner through the row's LDS region, X[M] in the element behind the data, inside the region's padding;
//     Z'[k] = (A + B) + i conj(W_n^k) (A - B);  z = the un-normalised inverse DFT_M(Z');
//     y[2p] = w[2p] Re z[p] / n, y[2p+1] = w[2p+1] Im z[p] / n: one 8-byte store per element.  1 / n is a power of two: exact.
//
// Twiddles: W_n^k (k < M) is the row that the DCT kernels build at compile time from the fp64-rounded first octant of W_32768
// (smfft_twiddles_dct.inc) by exact symmetries (smfft_rows.hpp), in an object of this library's own so that the other libraries and
// their kernels stay as they are.  No v_sin / v_cos.
//
// Cache policy, by measurement (tools/ab_stft.py, profiles/r25_stft_ab.txt): the sample loads of the forward
// kernels are plain -- overlapping frames fetch a sample from HBM once and from L2 after that, and at hop = n / 4 the launch with
// non-temporal loads takes 1.05 ... 1.22 times as long; at hop = n it takes 0.96 ... 0.99.  The loads of the inverse kernel's bins,
// which are read once, and all stores are non-temporal.  -DSMFFT_STFT_NT_LOAD / -DSMFFT_STFT_NT_BINS / -DSMFFT_STFT_NT_STORE = 1 / 0
// build each of the three non-temporal / plain; STFT_NT in the Makefile sets all three.  The window is always loaded plain: every
// frame reads it.
//
// -ffp-contract=on (Makefile, STFT_FLAGS_<M>): a product is fused into a sum only where one expression of the source writes both, so
// every build of this file rounds alike, the A/B builds give the shipped build's bits and the power kernel squares the complex
// kernel's values.  The windowed samples are products of their own statement, for that reason.
#include <hip/hip_runtime.h>

#include "smfft_stft.h"

namespace smfft {
namespace stft {
// enqueue `grid` workgroups on `stream`; 0 or the launch's hipError_t.  Defined per M by the objects compiled with -DSMFFT_STFT_N.
template <int M>
int launch_stft(const float* in, float* out, const float* window, long long total, long long frames, long long hop, long long stream_stride, int kind,
                int grid, hipStream_t stream);
template <int M>
int launch_istft(const float2* in, float* out, const float* window, long long batch, int grid, hipStream_t stream);
}  // namespace stft
}  // namespace smfft

#ifdef SMFFT_STFT_N
#include "smfft_fir_kernel.hpp"
#include "smfft_rows.hpp"

// the policy of the sample loads (forward), of the loads of the bins (inverse) and of the stores: 1 non-temporal, 0 plain
#ifndef SMFFT_STFT_NT_LOAD
#define SMFFT_STFT_NT_LOAD 0
#endif
#ifndef SMFFT_STFT_NT_BINS
#define SMFFT_STFT_NT_BINS SMFFT_NT
#endif
#ifndef SMFFT_STFT_NT_STORE
#define SMFFT_STFT_NT_STORE SMFFT_NT
#endif

namespace smfft {
namespace stft {

using rows::w32768, rows::row_entry, rows::per_tile;

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

// two consecutive floats at 4-byte alignment (samples, window) and one complex value at 8-byte alignment, with the policies above
__device__ __forceinline__ float2 gload2(const float* p) { return rows::gload2<SMFFT_STFT_NT_LOAD != 0>(p); }
__device__ __forceinline__ float2 gloadc(const float2* p) { return rows::gloadc<SMFFT_STFT_NT_BINS != 0>(p); }
// the window: plain loads, every frame reads it
__device__ __forceinline__ float2 wload2(const float* p) { return rows::gload2<false>(p); }
__device__ __forceinline__ void gstore1(float* p, float v) { rows::gstore1<SMFFT_STFT_NT_STORE != 0>(p, v); }
__device__ __forceinline__ void gstore2(float* p, float a, float b) { rows::gstore2<SMFFT_STFT_NT_STORE != 0>(p, a, b); }
__device__ __forceinline__ void gstorec(float2* p, float a, float b) { rows::gstorec<SMFFT_STFT_NT_STORE != 0>(p, a, b); }

// frame g = c frames + f < total reads in[c stream_stride + f hop ... + n), n = 2 M, under window[0, n) (null: all ones).
// KIND 0: out[2 (g (M + 1) + k)], out[2 (g (M + 1) + k) + 1] = Re, Im X[k]; KIND 1: out[g (M + 1) + k] = |X[k]|^2; k <= M
template <int M, int KIND>
__global__ void __launch_bounds__(kFirThreads) stft_kernel(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ window,
                                                           long long total, long long frames, long long hop, long long stream_stride) {
    using G = Geometry<M>;
    constexpr int T = G::T;
    __shared__ float2 s[G::kFftsPerBlock * G::SF];
    Engine<M, 0, 1> fwd;
    fwd.init(threadIdx.x);
    float2* sf = s + fwd.fft * G::SF;
    const long long ntiles = (total + G::kFftsPerBlock - 1) / G::kFftsPerBlock;
    const bool self = fwd.u == 0;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long g = tile * G::kFftsPerBlock + fwd.fft;
        const bool active = g < total;
        // an inactive slot of the last tile reads frame 0 and stores nothing
        const long long gg = active ? g : 0;
        const long long c = gg / frames;
        const float* xr = in + c * stream_stride + (gg - c * frames) * hop;
        float2 r[16], p[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) r[q] = gload2(xr + 2 * (fwd.u + T * q));
        if (window) {
            float2 w[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) w[q] = wload2(window + 2 * (fwd.u + T * q));
            // nothing is scheduled across this point: the loads all go out before the first arithmetic
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float v0 = r[q].x * w[q].x;
                const float v1 = r[q].y * w[q].y;
                r[q] = make_float2(v0, v1);
            }
        } else {
            __builtin_amdgcn_sched_barrier(0);
        }
        fft_sync<G::kMultiWave>();             // the previous tile's partner reads are done with the region
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
        const float x0 = p[0].x + p[0].y, xm = p[0].x - p[0].y;
        r[0] = self ? make_float2(x0, 0.f) : r[0];
        if constexpr (KIND == 0) {
            float2* yr = reinterpret_cast<float2*>(out) + g * (M + 1);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                if (active) gstorec(yr + (fwd.u + T * q), r[q].x, r[q].y);
            }
            if (active && self) gstorec(yr + M, xm, 0.f);
        } else {
            float* yr = out + g * (M + 1);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float pw = r[q].x * r[q].x + r[q].y * r[q].y;
                if (active) gstore1(yr + (fwd.u + T * q), pw);
            }
            const float pm = xm * xm;          // + 0 * 0
            if (active && self) gstore1(yr + M, pm);
        }
    }
}

// out[r n + j] = window[j] irfft_n(in[r (M + 1) ... + M + 1))[j], n = 2 M (window null: all ones)
template <int M>
__global__ void __launch_bounds__(kFirThreads) istft_kernel(const float2* __restrict__ in, float* __restrict__ out, const float* __restrict__ window,
                                                            long long batch) {
    using G = Geometry<M>;
    constexpr int T = G::T, n = 2 * M;
    __shared__ float2 s[G::kFftsPerBlock * G::SF];
    Engine<M, 1, 1> inv;
    inv.init(threadIdx.x);
    float2* sf = s + inv.fft * G::SF;
    const long long ntiles = (batch + G::kFftsPerBlock - 1) / G::kFftsPerBlock;
    const bool self = inv.u == 0;
    const float scale = 1.f / (float)n;        // the inverse transform is un-normalised.  An exact power of two
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long g = tile * G::kFftsPerBlock + inv.fft;
        const bool active = g < batch;
        // an inactive slot of the last tile reads row 0 and stores nothing
        const float2* xr = in + (active ? g : 0) * (M + 1);
        float2 r[16], p[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) r[q] = gloadc(xr + (inv.u + T * q));
        float2 top = make_float2(0.f, 0.f);
        if (self) top = gloadc(xr + M);
        // nothing is scheduled across this point: the loads all go out before the first arithmetic
        __builtin_amdgcn_sched_barrier(0);
        fft_sync<G::kMultiWave>();             // the previous tile's inverse transform is done with the region
#pragma unroll
        for (int q = 0; q < 16; ++q) sf[inv.u + T * q] = r[q];
        if (self) sf[M] = top;                 // X[M], behind the data: inside the region's padding (SF = 17 M / 16)
        fft_sync<G::kMultiWave>();
        // X[M - (u + T q)] = X[(T - u) + T (15 - q)]; thread 0's q = 0 reads X[M]
        const float2* partner = sf + (T - inv.u);
#pragma unroll
        for (int q = 0; q < 16; ++q) p[q] = partner[T * (15 - q)];
        // the two real bins: their imaginary parts are ignored
        r[0].y = self ? 0.f : r[0].y;
        p[0].y = self ? 0.f : p[0].y;
        const int u = per_tile(inv.u);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float2 w = row_entry(&rows<M>.wn[u + T * q]);        // (c, s): conj W_n^k = c + i s
            // B = conj p; S = A + B, D = A - B; Z' = S + i (c + i s) D
            const float sx = r[q].x + p[q].x, sy = r[q].y - p[q].y, dx = r[q].x - p[q].x, dy = r[q].y + p[q].y;
            r[q] = make_float2(sx - w.y * dx - w.x * dy, sy + w.x * dx - w.y * dy);
        }
        fft_sync<G::kMultiWave>();             // the partner reads are done
        inv.transform(r, sf);
        // the window, or ones (a product with one is exact): one store path
        float2 w[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) w[q] = make_float2(1.f, 1.f);
        if (window) {
#pragma unroll
            for (int q = 0; q < 16; ++q) w[q] = wload2(window + 2 * (inv.u + T * q));
        }
        float* yr = out + g * n;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float y0 = scale * r[q].x, y1 = scale * r[q].y;
            const float v0 = y0 * w[q].x;
            const float v1 = y1 * w[q].y;
            if (active) gstore2(yr + 2 * (inv.u + T * q), v0, v1);
        }
    }
}

template <>
int launch_stft<SMFFT_STFT_N>(const float* in, float* out, const float* window, long long total, long long frames, long long hop, long long stream_stride,
                              int kind, int grid, hipStream_t stream) {
    const dim3 blocks((unsigned)grid), threads(kFirThreads);
    if (kind == 0) hipLaunchKernelGGL((stft_kernel<SMFFT_STFT_N, 0>), blocks, threads, 0, stream, in, out, window, total, frames, hop, stream_stride);
    else hipLaunchKernelGGL((stft_kernel<SMFFT_STFT_N, 1>), blocks, threads, 0, stream, in, out, window, total, frames, hop, stream_stride);
    return (int)hipGetLastError();
}

template <>
int launch_istft<SMFFT_STFT_N>(const float2* in, float* out, const float* window, long long batch, int grid, hipStream_t stream) {
    hipLaunchKernelGGL(istft_kernel<SMFFT_STFT_N>, dim3((unsigned)grid), dim3(kFirThreads), 0, stream, in, out, window, batch);
    return (int)hipGetLastError();
}

}  // namespace stft
}  // namespace smfft

#else  // the C ABI
#include "smfft_rows_host.hpp"

namespace {
constexpr unsigned long long kMaxElements = 1ull << 59;      // floats of a buffer: keeps the byte counts below inside 64 bits

// the launches of `grid` workgroups (<= 0: the default) on `stream`
auto dispatch_stft(const void* in, void* out, const void* window, int n, long long streams, long long frames, long long hop, long long stream_stride,
                   int kind) {
    return [=](int grid, hipStream_t stream) {
        const int M = half_length_fft_size(n);
        const long long total = streams * frames;
        grid = default_grid(M, total, grid);
        return dispatch_m(M, [&](auto m) {
            return smfft::stft::launch_stft<m()>((const float*)in, (float*)out, (const float*)window, total, frames, hop, stream_stride, kind, grid, stream);
        });
    };
}

auto dispatch_istft(const void* in, void* out, const void* window, int n, long long batch) {
    return [=](int grid, hipStream_t stream) {
        const int M = half_length_fft_size(n);
        grid = default_grid(M, batch, grid);
        return dispatch_m(M, [&](auto m) { return smfft::stft::launch_istft<m()>((const float2*)in, (float*)out, (const float*)window, batch, grid, stream); });
    };
}

// -1: refused; 0: launch; 1: nothing to do.  No HIP call.
// stft: the output overlaps neither the range of the frames nor the window
int check_stft(const void* in, const void* out, const void* window, int n, long long streams, long long frames, long long hop, long long stream_stride,
               int kind) {
    const int M = half_length_fft_size(n);
    if (M < 0 || kind < 0 || kind > 1 || streams < 0 || frames < 0 || hop < 1 || stream_stride < 1) return -1;
    if (streams == 0 || frames == 0) return 1;
    const unsigned __int128 total = (unsigned __int128)streams * (unsigned __int128)frames;
    const unsigned __int128 extent = (unsigned __int128)(streams - 1) * (unsigned __int128)stream_stride
                                     + (unsigned __int128)(frames - 1) * (unsigned __int128)hop + (unsigned)n;
    if (total > kMaxElements / (unsigned)n || extent > kMaxElements) return -1;
    // floats of the output: M + 1 complex values or M + 1 powers per frame
    const unsigned long long outs = (unsigned long long)total * (unsigned)(M + 1) * (kind == 0 ? 2u : 1u);
    if (overlap(in, (unsigned long long)extent, out, outs)) return -1;
    if (window && overlap(window, (unsigned)n, out, outs)) return -1;
    return 0;
}

// istft: the output overlaps neither the input nor the window
int check_istft(const void* in, const void* out, const void* window, int n, long long batch) {
    const int M = half_length_fft_size(n);
    if (M < 0 || batch < 0) return -1;
    if (batch == 0) return 1;
    if ((unsigned long long)batch > kMaxElements / (2u * (unsigned)n)) return -1;
    const unsigned long long ins = (unsigned long long)batch * (unsigned)(M + 1) * 2u, outs = (unsigned long long)batch * (unsigned)n;
    if (overlap(in, ins, out, outs)) return -1;
    if (window && overlap(window, (unsigned)n, out, outs)) return -1;
    return 0;
}
}  // namespace

extern "C" {

int smfft_stft_fft_size(int n) { return half_length_fft_size(n); }

long long smfft_stft_frames(long long L, int n, long long hop) {
    if (half_length_fft_size(n) < 0 || hop < 1 || L < 0) return -1;
    return L < n ? 0 : 1 + (L - n) / hop;
}

int smfft_stft_launch(const void* d_in, void* d_out, const void* d_window, int n, long long streams, long long frames, long long hop, long long stream_stride, int kind, void* hip_stream) {
    return checked_launch(check_stft(d_in, d_out, d_window, n, streams, frames, hop, stream_stride, kind),
                          dispatch_stft(d_in, d_out, d_window, n, streams, frames, hop, stream_stride, kind), hip_stream);
}

int smfft_stft_launch_tuned(const void* d_in, void* d_out, const void* d_window, int n, long long streams, long long frames, long long hop, long long stream_stride, int kind, void* hip_stream, int grid) {
    return checked_launch_tuned(check_stft(d_in, d_out, d_window, n, streams, frames, hop, stream_stride, kind),
                                dispatch_stft(d_in, d_out, d_window, n, streams, frames, hop, stream_stride, kind), hip_stream, grid);
}

int smfft_stft_benchmark(const void* d_in, void* d_out, const void* d_window, int n, long long streams, long long frames, long long hop, long long stream_stride, int kind, double* FFT_time) {
    return checked_benchmark(check_stft(d_in, d_out, d_window, n, streams, frames, hop, stream_stride, kind),
                             dispatch_stft(d_in, d_out, d_window, n, streams, frames, hop, stream_stride, kind), FFT_time);
}

int smfft_istft_launch(const void* d_in, void* d_out, const void* d_window, int n, long long batch, void* hip_stream) {
    return checked_launch(check_istft(d_in, d_out, d_window, n, batch), dispatch_istft(d_in, d_out, d_window, n, batch), hip_stream);
}

int smfft_istft_launch_tuned(const void* d_in, void* d_out, const void* d_window, int n, long long batch, void* hip_stream, int grid) {
    return checked_launch_tuned(check_istft(d_in, d_out, d_window, n, batch), dispatch_istft(d_in, d_out, d_window, n, batch), hip_stream, grid);
}

int smfft_istft_benchmark(const void* d_in, void* d_out, const void* d_window, int n, long long batch, double* FFT_time) {
    return checked_benchmark(check_istft(d_in, d_out, d_window, n, batch), dispatch_istft(d_in, d_out, d_window, n, batch), FFT_time);
}

}  // extern "C"
#endif

// smfft_czt.hip -- libsmfft_czt.so: batched chirp-z (zoom) transforms, m points on an arc of the unit circle from rows of n samples
// (n, m <= 2048), on the register engine's transforms of M = 256 ... 4096 points, in one kernel and one pass through HBM, and the C ABI
// of include/smfft_czt.h.
//
// Compiled once per M (Makefile: -DSMFFT_CZT_N=256 ... 4096, flags of their own: CZT_FLAGS_<M>) for the kernel and its launcher, and
// once without SMFFT_CZT_N for the C ABI, which checks, builds the tables (smfft_czt_tables.hpp, fp64 on the host) and dispatches.
//
// czt_kernel<M> is smfft_bluestein.hip's chain (DESIGN.md sections 18 and 19) without its three shortcuts: the chirp behind the load
// (A, which carries `start`) and the one in front of the store (C) are two tables; a row has n inputs and m outputs; and M >= n + m - 1
// lets either of n, m exceed M / 2, so a thread loads, transforms and stores all sixteen of its elements u + T q and holds sixteen
// elements of each of A, B and C.  The three tables are the same for every row: at M <= 1024 a thread loads its 48 elements once, in
// front of the tile loop, and keeps them in registers across the grid-stride loop.  At M = 2048 and 4096 that came to 266 and 276
// registers, one wave per SIMD, so there C is staged once per workgroup in LDS behind the transform region instead (M float2 more: 51,200
// and 67,584 B, still two workgroups per compute unit) and read at the store.  The body is written out in the kernel itself, for the
// reason smfft_fir_kernel.hpp gives.
//
// The row loads and stores are the engine's gload / gstore: non-temporal, as in the FIR banks.  -DSMFFT_NT=0 (make
// EXTRA_HIPFLAGS=-DSMFFT_NT=0 CZT_LIB=... CZT_OBJDIR=...) builds them plain for the A/B of tools/ab_czt.py.
#include <hip/hip_runtime.h>

#include "smfft_czt.h"

namespace smfft {
namespace czt {
// enqueue `grid` workgroups on `stream`; 0 or the launch's hipError_t.  Defined per M by the objects compiled with -DSMFFT_CZT_N.
template <int M>
int launch_rows(const float2* in, float2* out, int n, int m, long long batch, const float2* plan, int grid, hipStream_t stream);
}  // namespace czt
}  // namespace smfft

#ifdef SMFFT_CZT_N
#include "smfft_fir_kernel.hpp"

namespace smfft {
namespace czt {

// out[r m + k] = C[k] IDFT_M(DFT_M(pad_M(in[r n + .] A)) B)[k], k < m: the m points of the plan's arc of row r.
// in and out may be the same buffer when m == n: no __restrict__ on them.
template <int M>
__global__ void __launch_bounds__(kFirThreads) czt_kernel(const float2* in, float2* out, const float2* __restrict__ plan, int n, int m, long long batch) {
    using G = Geometry<M>;
    // M >= 2048: 96 registers of tables beside the transform's do not fit into 256, so C lives in LDS behind the transform region
    // (one copy per workgroup, read at the store) and two workgroups per compute unit still fit
    constexpr bool kCInLds = M >= 2048;
    __shared__ float2 s[G::kFftsPerBlock * G::SF + (kCInLds ? M : 0)];
    Engine<M, 0, 1> fwd;
    Engine<M, 1, 1> inv;
    fwd.init(threadIdx.x);
    inv.init(threadIdx.x);
    float2* sf = s + fwd.fft * G::SF;
    const long long ntiles = (batch + G::kFftsPerBlock - 1) / G::kFftsPerBlock;
    // the input chirp, the spectrum of the kernel b and the output chirp: the same for every row, loaded once per workgroup
    float2 a[16], h[16], c[kCInLds ? 1 : 16];
    float2* sc = s + G::kFftsPerBlock * G::SF;
#pragma unroll
    for (int q = 0; q < 16; ++q) a[q] = plan[fwd.u + G::T * q];
#pragma unroll
    for (int q = 0; q < 16; ++q) h[q] = plan[M + fwd.u + G::T * q];
    if constexpr (kCInLds) {
        for (int i = threadIdx.x; i < M; i += kFirThreads) sc[i] = plan[2 * M + i];
        __syncthreads();
    } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) c[q] = plan[2 * M + fwd.u + G::T * q];
    }
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long g = tile * G::kFftsPerBlock + fwd.fft;
        const bool active = g < batch;
        // in[r n + j], zero at j >= n: a clamped in-range address and a select afterwards, so the loads go out back to back; an inactive
        // slot of the last tile reads row 0 and stores nothing
        const float2* xr = in + (active ? g : 0) * n;
        float2 r[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int j = fwd.u + G::T * q;
            const int jc = j < n ? j : n - 1;
            const float2 v = gload(xr + jc);
            r[q] = cmul_fixed((j == jc) ? v : make_float2(0.f, 0.f), a[q]);
        }
        fft_sync<G::kMultiWave>();             // the previous tile's inverse transform is done with the region
        fwd.transform(r, sf);
#pragma unroll
        for (int q = 0; q < 16; ++q) r[q] = cmul_fixed(r[q], h[q]);
        fft_sync<G::kMultiWave>();             // the forward transform's last LDS reads are done
        inv.transform(r, sf);
        float2* yr = out + g * m;
        const int kend = active ? m : 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int k = fwd.u + G::T * q;
            // + 0: a product of a zero with a negative component of C is -0, and a row of zeros transforms to +0 in every element
            const float2 v = cmul_fixed(r[q], kCInLds ? sc[k] : c[q]);
            if (k < kend) gstore(yr + k, make_float2(v.x + 0.f, v.y + 0.f));
        }
    }
}

template <>
int launch_rows<SMFFT_CZT_N>(const float2* in, float2* out, int n, int m, long long batch, const float2* plan, int grid, hipStream_t stream) {
    hipLaunchKernelGGL(czt_kernel<SMFFT_CZT_N>, dim3((unsigned)grid), dim3(kFirThreads), 0, stream, in, out, plan, n, m, batch);
    return (int)hipGetLastError();
}

}  // namespace czt
}  // namespace smfft

#else  // the C ABI
#include <cmath>
#include <vector>

#include "smfft_czt_tables.hpp"
#include "smfft_rows_host.hpp"

namespace {
// the launch of `grid` workgroups (<= 0: the default) on `stream`
auto dispatch(const void* in, void* out, int n, int m, long long batch, const void* plan) {
    return [=](int grid, hipStream_t stream) {
        const int M = smfft::czt::fft_size(n, m);
        grid = default_grid(M, batch, grid);
        return dispatch_m(M, [&](auto len) { return smfft::czt::launch_rows<len()>((const float2*)in, (float2*)out, n, m, batch, (const float2*)plan, grid, stream); });
    };
}

// -1: refused; 0: launch; 1: nothing to do.  No HIP call.  In place only with m == n: rows of another length overlap their neighbours'.
int check(const void* in, const void* out, int n, int m, long long batch) {
    if (smfft::czt::fft_size(n, m) < 0 || batch < 0 || (out == in && m != n)) return -1;
    return batch == 0 ? 1 : 0;
}

bool arc_ok(double start, double step) { return std::isfinite(start) && std::isfinite(step); }
}  // namespace

extern "C" {

int smfft_czt_fft_size(int n, int m) { return smfft::czt::fft_size(n, m); }

long long smfft_czt_plan_bytes(int n, int m) {
    const int M = smfft::czt::fft_size(n, m);
    return M < 0 ? -1 : 24LL * M;
}

int smfft_czt_tables(int n, int m, double start, double step, void* h_plan) {
    if (smfft::czt::fft_size(n, m) < 0 || !arc_ok(start, step) || !h_plan) return -1;
    smfft::czt::build_tables(n, m, start, step, (float*)h_plan);
    return 0;
}

int smfft_czt_prepare(int n, int m, double start, double step, void* d_plan, void* hip_stream) {
    const int M = smfft::czt::fft_size(n, m);
    if (M < 0 || !arc_ok(start, step)) return -1;
    std::vector<float> plan(6 * (size_t)M);
    smfft::czt::build_tables(n, m, start, step, plan.data());
    int rc = (int)hipMemcpyAsync(d_plan, plan.data(), plan.size() * sizeof(float), hipMemcpyHostToDevice, (hipStream_t)hip_stream);
    if (rc == 0) rc = (int)hipStreamSynchronize((hipStream_t)hip_stream);      // the host copy of the plan ends with this call
    return rc;
}

int smfft_czt_launch(const void* d_in, void* d_out, int n, int m, long long batch, const void* d_plan, void* hip_stream) {
    return checked_launch(check(d_in, d_out, n, m, batch), dispatch(d_in, d_out, n, m, batch, d_plan), hip_stream);
}

int smfft_czt_launch_tuned(const void* d_in, void* d_out, int n, int m, long long batch, const void* d_plan, void* hip_stream, int grid) {
    return checked_launch_tuned(check(d_in, d_out, n, m, batch), dispatch(d_in, d_out, n, m, batch, d_plan), hip_stream, grid);
}

int smfft_czt_benchmark(const void* d_in, void* d_out, int n, int m, long long batch, const void* d_plan, double* FFT_time) {
    return checked_benchmark(check(d_in, d_out, n, m, batch), dispatch(d_in, d_out, n, m, batch, d_plan), FFT_time);
}

}  // extern "C"
#endif

// smfft_bluestein.hip -- libsmfft_bluestein.so: batched C2C FFTs of any length 1 <= n <= 2048 by Bluestein's algorithm on the register
// engine's transforms of M = 256 ... 4096 points, in one kernel and one pass through HBM, and the C ABI of include/smfft_bluestein.h.
//
// Compiled once per M (Makefile: -DSMFFT_BLUESTEIN_N=256 ... 4096, flags of their own: BLUESTEIN_FLAGS_<M>) for the kernel and its
// launcher, and once without SMFFT_BLUESTEIN_N for the C ABI, which checks, builds the tables (smfft_bluestein_tables.hpp, fp64 on the
// host) and dispatches.
//
// bluestein_kernel<M> is smfft_fir_detect.hip's fir_power_kernel with ONE fixed filter: the same clamped loads,
// forward transform, product with a prepared spectrum in registers, inverse transform and windowed store, plus a unit-modulus multiply
// behind the load and in front of the store.  The two tables are the same for every row, so a thread loads its elements of them once,
// in front of the tile loop, and keeps them in registers across the grid-stride loop.  The body is written out in the kernel itself, for
// the reason smfft_fir_kernel.hpp gives.
//
// M >= 2n - 1 makes n <= M / 2: the elements j = u + T q with q >= 8 lie at j >= M / 2 >= n, whatever n is.  They are zero in front of
// the forward transform and are not stored behind the inverse one, so a thread loads and stores its eight lower elements only, and
// holds eight elements of W.
//
// The row loads and stores are the engine's gload / gstore: non-temporal, as in the FIR banks.  -DSMFFT_NT=0 (make
// EXTRA_HIPFLAGS=-DSMFFT_NT=0 BLUESTEIN_LIB=... BLUESTEIN_OBJDIR=...) builds them plain for the A/B of tools/ab_bluestein.py, which
// finds a tie.
#include <hip/hip_runtime.h>

#include "smfft_bluestein.h"

namespace smfft {
namespace bluestein {
// enqueue `grid` workgroups on `stream`; 0 or the launch's hipError_t.  Defined per M by the objects compiled with -DSMFFT_BLUESTEIN_N.
template <int M>
int launch_rows(const float2* in, float2* out, int n, long long batch, const float2* plan, int grid, hipStream_t stream);
}  // namespace bluestein
}  // namespace smfft

#ifdef SMFFT_BLUESTEIN_N
#include "smfft_fir_kernel.hpp"

namespace smfft {
namespace bluestein {

// out[r n + k] = W[k] IDFT_M(DFT_M(pad_M(in[r n + .] W)) B)[k], k < n: the DFT of n points of row r in the direction of the plan.
// in and out may be the same buffer: no __restrict__ on them.
template <int M>
__global__ void __launch_bounds__(kFirThreads) bluestein_kernel(const float2* in, float2* out, const float2* __restrict__ plan, int n, long long batch) {
    using G = Geometry<M>;
    constexpr int kHalf = 8;           // the elements q < 8 of a thread are those below M / 2
    __shared__ float2 s[G::kFftsPerBlock * G::SF];
    Engine<M, 0, 1> fwd;
    Engine<M, 1, 1> inv;
    fwd.init(threadIdx.x);
    inv.init(threadIdx.x);
    float2* sf = s + fwd.fft * G::SF;
    const long long ntiles = (batch + G::kFftsPerBlock - 1) / G::kFftsPerBlock;
    // the chirp and the spectrum of its mirror image: the same for every row, loaded once per workgroup
    float2 w[kHalf], h[16];
#pragma unroll
    for (int q = 0; q < kHalf; ++q) w[q] = plan[fwd.u + G::T * q];
#pragma unroll
    for (int q = 0; q < 16; ++q) h[q] = plan[M + fwd.u + G::T * q];
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long g = tile * G::kFftsPerBlock + fwd.fft;
        const bool active = g < batch;
        // in[r n + j], zero at j >= n: a clamped in-range address and a select afterwards, so the loads go out back to back; an inactive
        // slot of the last tile reads row 0 and stores nothing
        const float2* xr = in + (active ? g : 0) * n;
        float2 r[16];
#pragma unroll
        for (int q = 0; q < kHalf; ++q) {
            const int j = fwd.u + G::T * q;
            const int jc = j < n ? j : n - 1;
            const float2 v = gload(xr + jc);
            r[q] = cmul_fixed((j == jc) ? v : make_float2(0.f, 0.f), w[q]);
        }
#pragma unroll
        for (int q = kHalf; q < 16; ++q) r[q] = make_float2(0.f, 0.f);
        fft_sync<G::kMultiWave>();             // the previous tile's inverse transform is done with the region
        fwd.transform(r, sf);
#pragma unroll
        for (int q = 0; q < 16; ++q) r[q] = cmul_fixed(r[q], h[q]);
        fft_sync<G::kMultiWave>();             // the forward transform's last LDS reads are done
        inv.transform(r, sf);
        float2* yr = out + g * n;
        const int jend = active ? n : 0;
#pragma unroll
        for (int q = 0; q < kHalf; ++q) {
            const int j = fwd.u + G::T * q;
            // + 0: a product of a zero with a negative component of W is -0, and a row of zeros transforms to +0 in every element
            const float2 v = cmul_fixed(r[q], w[q]);
            if (j < jend) gstore(yr + j, make_float2(v.x + 0.f, v.y + 0.f));
        }
    }
}

template <>
int launch_rows<SMFFT_BLUESTEIN_N>(const float2* in, float2* out, int n, long long batch, const float2* plan, int grid, hipStream_t stream) {
    hipLaunchKernelGGL(bluestein_kernel<SMFFT_BLUESTEIN_N>, dim3((unsigned)grid), dim3(kFirThreads), 0, stream, in, out, plan, n, batch);
    return (int)hipGetLastError();
}

}  // namespace bluestein
}  // namespace smfft

#else  // the C ABI
#include <vector>

#include "smfft_bluestein_tables.hpp"
#include "smfft_rows_host.hpp"

namespace {
// the launch of `grid` workgroups (<= 0: the default) on `stream`
auto dispatch(const void* in, void* out, int n, long long batch, const void* plan) {
    return [=](int grid, hipStream_t stream) {
        const int M = smfft::bluestein::fft_size(n);
        grid = default_grid(M, batch, grid);
        return dispatch_m(M, [&](auto m) { return smfft::bluestein::launch_rows<m()>((const float2*)in, (float2*)out, n, batch, (const float2*)plan, grid, stream); });
    };
}

// -1: refused; 0: launch; 1: nothing to do.  No HIP call.
int check(int n, long long batch) {
    if (smfft::bluestein::fft_size(n) < 0 || batch < 0) return -1;
    return batch == 0 ? 1 : 0;
}
}  // namespace

extern "C" {

int smfft_bluestein_fft_size(int n) { return smfft::bluestein::fft_size(n); }

long long smfft_bluestein_plan_bytes(int n) {
    const int M = smfft::bluestein::fft_size(n);
    return M < 0 ? -1 : 16LL * M;
}

int smfft_bluestein_tables(int n, int inverse, void* h_plan) {
    if (smfft::bluestein::fft_size(n) < 0 || !h_plan) return -1;
    smfft::bluestein::build_tables(n, inverse != 0, (float*)h_plan);
    return 0;
}

int smfft_bluestein_prepare(int n, int inverse, void* d_plan, void* hip_stream) {
    const int M = smfft::bluestein::fft_size(n);
    if (M < 0) return -1;
    std::vector<float> plan(4 * (size_t)M);
    smfft::bluestein::build_tables(n, inverse != 0, plan.data());
    int rc = (int)hipMemcpyAsync(d_plan, plan.data(), plan.size() * sizeof(float), hipMemcpyHostToDevice, (hipStream_t)hip_stream);
    if (rc == 0) rc = (int)hipStreamSynchronize((hipStream_t)hip_stream);      // the host copy of the plan ends with this call
    return rc;
}

int smfft_bluestein_launch(const void* d_in, void* d_out, int n, long long batch, const void* d_plan, void* hip_stream) {
    return checked_launch(check(n, batch), dispatch(d_in, d_out, n, batch, d_plan), hip_stream);
}

int smfft_bluestein_launch_tuned(const void* d_in, void* d_out, int n, long long batch, const void* d_plan, void* hip_stream, int grid) {
    return checked_launch_tuned(check(n, batch), dispatch(d_in, d_out, n, batch, d_plan), hip_stream, grid);
}

int smfft_bluestein_benchmark(const void* d_in, void* d_out, int n, long long batch, const void* d_plan, double* FFT_time) {
    return checked_benchmark(check(n, batch), dispatch(d_in, d_out, n, batch, d_plan), FFT_time);
}

}  // extern "C"
#endif

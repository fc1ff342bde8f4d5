// smfft_pfb_real.hip -- libsmfft_pfb_real.so: the critically sampled polyphase filter bank channelizer for REAL streams (weighted sum over
// the P polyphase branches of frames of 2N real samples + the 2N-point real-to-complex transform, in one kernel) and the C ABI of
// include/smfft_pfb_real.h.
//
// Compiled once per length (Makefile: -DSMFFT_PFB_REAL_N=256 ... 4096, flags of their own: PFB_REAL_FLAGS_<N>) for the kernels and their
// launcher, and once without SMFFT_PFB_REAL_N for the C ABI, which only checks and dispatches.
//
// The kernel is smfft_pfb_kernel.hpp's pfb_body -- the loop, the schedule, the transform and the store that both filter banks share --
// on float2 = two consecutive real samples: a frame of 2N reals is N float2, so the plan is smfft::PfbPlan{L / 2, N, P, C} in float2
// units, unchanged.  With the bank of smfft_pfb_real_bank.hpp (shared with smfft_pfb_spec.hip) a thread accumulates the PACKED sequence
//     z[n] = w[2n] + i w[2n + 1],   w[m] = sum_p h[2 p N + m] x[(f + p) 2N + m],   n = u + T c
// -- per tap, after the sixteen signal loads, the sixteen coefficient PAIRS (h[2n], h[2n + 1]) as 8-byte loads, then one fused
// multiply-add per component --, and after the transform (r[q] = Z[u + T q]) it splits Z into the spectrum of the real frame X[k],
// 0 <= k < N, with X[N] packed into the imaginary part of element 0 (the layout of the R2C kernels of libsmfft_amd.so).  The split is the
// R2C external kernels' own (smfft_kernels.hpp): HermitianRegisters<N, 0> -- partner values through ds_bpermute, no LDS memory -- for FFTs that live in one wave,
// hermitian_pass's body (hermitian_pass_with: the twiddle handed in) through the FFT's LDS region otherwise; N = 4096 needs W_8192^i,
// which the 4096-entry table does not hold: they are built at compile time from the fp64-rounded octant of W_16384, as smfft_large.hpp
// builds its rows.
//
// -DSMFFT_PFB_REAL_SPLIT=0 / 1: the split through LDS / in registers at every length that can do either (N <= 1024: one wave per FFT).
// -DSMFFT_PFB_REAL_NT_LOADS=0 / 1: the signal loads plain / non-temporal.  Build variables for the A/B of tools/ab_pfb_real.py (a second
// library beside the shipped one), not run-time branches; the defaults are below.
#include <hip/hip_runtime.h>

#include "smfft_pfb.hpp"
#include "smfft_pfb_real.h"

namespace smfft {
namespace pfb_real {
// the bank as the C ABI half sees it (smfft_pfb_host.hpp)
struct Host {
    static constexpr int kSamplesPerElement = 2;       // a float2 of the plan is two real samples: a frame of 2N reals is N float2, L even
    // enqueue on `stream`; plan in float2 units; cus = compute units of the current device; R = the schedule's run length; 0 or the
    // launch's hipError_t.  Defined per length by the objects compiled with -DSMFFT_PFB_REAL_N.
    template <int N>
    static int launch(const void* x, const void* h, void* y, const PfbPlan& plan, int power, long long R, int cus, hipStream_t stream);
};
}  // namespace pfb_real
}  // namespace smfft

#ifdef SMFFT_PFB_REAL_N
#include "smfft_pfb_real_bank.hpp"

namespace smfft {
namespace pfb_real {

template <int N, int POWER>
__global__ void __launch_bounds__(kPfbThreads) __attribute__((amdgpu_waves_per_eu(3, 3)))
pfb_real_kernel(const float2* __restrict__ x, const float2* __restrict__ h, void* __restrict__ y, PfbPlan plan, long long R) {
    __shared__ float2 s[Geometry<N>::kFftsPerBlock * Geometry<N>::SF];
    pfb_body<N, POWER, Bank>(x, h, y, plan, R, s);
}

template <>
int Host::launch<SMFFT_PFB_REAL_N>(const void* x, const void* h, void* y, const PfbPlan& plan, int power, long long R, int cus, hipStream_t stream) {
    return pfb_launch(pfb_real_kernel<SMFFT_PFB_REAL_N, 0>, pfb_real_kernel<SMFFT_PFB_REAL_N, 1>, (const float2*)x, (const float2*)h, y, plan, power, R, cus, stream);
}

}  // namespace pfb_real
}  // namespace smfft

#else  // the C ABI
#include "smfft_pfb_host.hpp"

using Api = PfbApi<smfft::pfb_real::Host>;

extern "C" {

long long smfft_pfb_real_frames(long long signal_length, int n_channels, int taps_per_channel) { return Api::frames(signal_length, n_channels, taps_per_channel); }

int smfft_pfb_real_default_tile_run(int n_channels, int taps_per_channel) { return Api::default_tile_run_or_error(n_channels, taps_per_channel); }

int smfft_pfb_real_launch_tuned(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                                int power, void* d_output, void* hip_stream, int tile_run) {
    return Api::launch_tuned(d_signal, signal_length, n_streams, d_taps, n_channels, taps_per_channel, power, d_output, hip_stream, tile_run);
}

int smfft_pfb_real_launch(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                          int power, void* d_output, void* hip_stream) {
    return Api::launch_tuned(d_signal, signal_length, n_streams, d_taps, n_channels, taps_per_channel, power, d_output, hip_stream, 0);
}

int smfft_pfb_real_benchmark(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                             int power, void* d_output, double* FFT_time) {
    return Api::benchmark(d_signal, signal_length, n_streams, d_taps, n_channels, taps_per_channel, power, d_output, FFT_time);
}

}  // extern "C"
#endif

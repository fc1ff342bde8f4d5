// smfft_pfb.hip -- libsmfft_pfb.so: the critically sampled polyphase filter bank channelizer (weighted sum over the P polyphase branches
// + N-point forward FFT, in one kernel) and the C ABI of include/smfft_pfb.h.
//
// Compiled once per length (Makefile: -DSMFFT_PFB_N=256 ... 4096, flags of their own: PFB_FLAGS_<N>) for the kernels and their
// launcher, and once without SMFFT_PFB_N for the C ABI, which only checks and dispatches.
//
// The kernel is smfft_pfb_kernel.hpp's pfb_body -- the loop, the schedule, the transform and the store that both filter banks share --
// with the bank of smfft_pfb_bank.hpp (shared with smfft_pfb_spec.hip): per tap the sixteen float coefficients h[p N + u + T c] after the sixteen signal loads, then two fused
// multiply-adds per element, r[c] = sum_p h[p N + u + T c] x[(f + p) N + u + T c]; nothing between the transform and the store.
//
// -DSMFFT_PFB_NT_LOADS=0 / 1: the signal loads plain or non-temporal.  A build variable for the A/B of tools/ab_pfb.py (a second
// library beside the shipped one), not a run-time branch; the default is the library's gload policy until that A/B has been run
// (DESIGN.md section 12).
#include <hip/hip_runtime.h>

#include "smfft_pfb.hpp"
#include "smfft_pfb.h"

namespace smfft {
namespace pfb {
// the bank as the C ABI half sees it (smfft_pfb_host.hpp)
struct Host {
    static constexpr int kSamplesPerElement = 1;       // a float2 of the plan is one complex sample
    // enqueue on `stream`; plan in float2 units; cus = compute units of the current device; R = the schedule's run length; 0 or the
    // launch's hipError_t.  Defined per length by the objects compiled with -DSMFFT_PFB_N.
    template <int N>
    static int launch(const void* x, const void* h, void* y, const PfbPlan& plan, int power, long long R, int cus, hipStream_t stream);
};
}  // namespace pfb
}  // namespace smfft

#ifdef SMFFT_PFB_N
#include "smfft_pfb_bank.hpp"

namespace smfft {
namespace pfb {

template <int N, int POWER>
__global__ void __launch_bounds__(kPfbThreads) pfb_kernel(const float2* __restrict__ x, const float* __restrict__ h, void* __restrict__ y, PfbPlan plan, long long R) {
    __shared__ float2 s[Geometry<N>::kFftsPerBlock * Geometry<N>::SF];
    pfb_body<N, POWER, Bank>(x, h, y, plan, R, s);
}

template <>
int Host::launch<SMFFT_PFB_N>(const void* x, const void* h, void* y, const PfbPlan& plan, int power, long long R, int cus, hipStream_t stream) {
    return pfb_launch(pfb_kernel<SMFFT_PFB_N, 0>, pfb_kernel<SMFFT_PFB_N, 1>, (const float2*)x, (const float*)h, y, plan, power, R, cus, stream);
}

}  // namespace pfb
}  // namespace smfft

#else  // the C ABI
#include "smfft_pfb_host.hpp"

using Api = PfbApi<smfft::pfb::Host>;

extern "C" {

long long smfft_pfb_frames(long long signal_length, int n_channels, int taps_per_channel) { return Api::frames(signal_length, n_channels, taps_per_channel); }

int smfft_pfb_default_tile_run(int n_channels, int taps_per_channel) { return Api::default_tile_run_or_error(n_channels, taps_per_channel); }

int smfft_pfb_launch_tuned(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                           int power, void* d_output, void* hip_stream, int tile_run) {
    return Api::launch_tuned(d_signal, signal_length, n_streams, d_taps, n_channels, taps_per_channel, power, d_output, hip_stream, tile_run);
}

int smfft_pfb_launch(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                     int power, void* d_output, void* hip_stream) {
    return Api::launch_tuned(d_signal, signal_length, n_streams, d_taps, n_channels, taps_per_channel, power, d_output, hip_stream, 0);
}

int smfft_pfb_benchmark(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                        int power, void* d_output, double* FFT_time) {
    return Api::benchmark(d_signal, signal_length, n_streams, d_taps, n_channels, taps_per_channel, power, d_output, FFT_time);
}

}  // extern "C"
#endif

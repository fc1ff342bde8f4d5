// smfft_large_pfb.hip -- libsmfft_large_pfb.so: the polyphase filter bank channelizer for N = 8192 / 16384 channels (weighted sum over
// the P polyphase branches + the single-pass large engine's forward transform, in one kernel) and the C ABI of
// include/smfft_large_pfb.h.
//
// Compiled once per length (Makefile: -DSMFFT_LARGE_PFB_N=8192 / 16384, flags of their own: LARGE_PFB_FLAGS_<N>) for the kernels and
// their launcher, and once without SMFFT_LARGE_PFB_N for the C ABI, which only checks and dispatches.
//
// The persistent grid: G = min(pairs, max_workgroups, cus x LargeGeometry<N>::kWorkgroupsPerCu) workgroups, rounded down to a multiple
// of 8 for the XCD-blocked schedule (the stride schedule where that leaves none): include/smfft/smfft_large_pfb.hpp, LargePfbSchedule.
//
// -DSMFFT_LARGE_PFB_NT_LOADS=0 / 1: the signal loads plain or non-temporal.  A build variable for the A/B of tools/ab_large_pfb.py (a
// second library beside the shipped one), not a run-time branch; the default is that A/B's winner, plain loads: the P - 1 re-reads of a
// frame by neighbouring workgroups then hit in L2 (profiles/r14_large_pfb_ab.txt).
#include <hip/hip_runtime.h>

#include "smfft_pfb.hpp"
#include "smfft_large_pfb.h"

namespace smfft {
namespace large {
// enqueue on `stream`; form = the schedule (1 or 2); cus = compute units of the current device; max_workgroups > 0 caps the grid
// (0: what the device holds at once); 0 or the launch's hipError_t.  Defined per length by the objects compiled with
// -DSMFFT_LARGE_PFB_N.
template <int N>
int launch_pfb(const void* x, const void* h, void* y, const PfbPlan& plan, int power, int form, int cus, int max_workgroups, hipStream_t stream);
}  // namespace large
}  // namespace smfft

#ifdef SMFFT_LARGE_PFB_N
#include "smfft/smfft_large_pfb.hpp"

#ifndef SMFFT_LARGE_PFB_NT_LOADS
#define SMFFT_LARGE_PFB_NT_LOADS 0
#endif

namespace smfft {
namespace large {
template <>
int launch_pfb<SMFFT_LARGE_PFB_N>(const void* x, const void* h, void* y, const PfbPlan& plan, int power, int form, int cus, int max_workgroups,
                                  hipStream_t stream) {
    constexpr int N = SMFFT_LARGE_PFB_N;
    long long cap = (long long)cus * LargeGeometry<N>::kWorkgroupsPerCu;
    if (max_workgroups > 0 && max_workgroups < cap) cap = max_workgroups;
    const LargePfbSchedule sched = LargePfbSchedule::make(plan.pairs(), cap, form);
    const dim3 blocks((unsigned)sched.grid), threads(N / 16);
    if (power)
        hipLaunchKernelGGL((pfb_large<N, 1, SMFFT_LARGE_PFB_NT_LOADS>), blocks, threads, 0, stream, (const float2*)x, (const float*)h, y, plan, sched);
    else
        hipLaunchKernelGGL((pfb_large<N, 0, SMFFT_LARGE_PFB_NT_LOADS>), blocks, threads, 0, stream, (const float2*)x, (const float*)h, y, plan, sched);
    return (int)hipGetLastError();
}
}  // namespace large
}  // namespace smfft

#else  // the C ABI
#include "smfft_addon_host.hpp"

namespace {
bool supported(int N, int P) { return (N == 8192 || N == 16384) && P >= 1 && P <= 32; }

// The shipped schedule: the XCD-blocked form, for every (N, P) -- the faster one at both lengths under either load policy at P = 8
// (profiles/r14_large_pfb_ab.txt); other P have not been measured.
int default_schedule(int N, int P) {
    (void)N;
    (void)P;
    return 2;
}

// -1: an unsupported combination; 0: launch; 1: nothing to do (no whole frame).  No HIP call.
int check(long long L, int C, int N, int P, int schedule, int max_workgroups) {
    if (!supported(N, P) || C <= 0 || L < 0 || schedule < 0 || schedule > 2 || max_workgroups < 0) return -1;
    return smfft::PfbPlan{L, N, P, C}.frames() == 0 ? 1 : 0;
}

int dispatch(const void* x, long long L, int C, const void* h, int N, int P, int power, void* y, int schedule, int max_workgroups, hipStream_t stream) {
    const int cus = compute_units();
    if (cus <= 0) return (int)hipErrorNoDevice;
    const smfft::PfbPlan plan{L, N, P, C};
    const int form = schedule > 0 ? schedule : default_schedule(N, P);
    const int pw = power != 0;
    if (N == 8192) return smfft::large::launch_pfb<8192>(x, h, y, plan, pw, form, cus, max_workgroups, stream);
    return smfft::large::launch_pfb<16384>(x, h, y, plan, pw, form, cus, max_workgroups, stream);
}
}  // namespace

extern "C" {

long long smfft_large_pfb_frames(long long signal_length, int n_channels, int taps_per_channel) {
    return supported(n_channels, taps_per_channel) && signal_length >= 0 ? smfft::PfbPlan{signal_length, n_channels, taps_per_channel, 1}.frames() : -1;
}

int smfft_large_pfb_default_schedule(int n_channels, int taps_per_channel) {
    return supported(n_channels, taps_per_channel) ? default_schedule(n_channels, taps_per_channel) : -1;
}

int smfft_large_pfb_launch_tuned(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                                 int power, void* d_output, void* hip_stream, int schedule, int max_workgroups) {
    const int chk = check(signal_length, n_streams, n_channels, taps_per_channel, schedule, max_workgroups);
    if (chk != 0) return chk < 0 ? -1 : 0;
    return dispatch(d_signal, signal_length, n_streams, d_taps, n_channels, taps_per_channel, power, d_output, schedule, max_workgroups, (hipStream_t)hip_stream);
}

int smfft_large_pfb_launch(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                           int power, void* d_output, void* hip_stream) {
    return smfft_large_pfb_launch_tuned(d_signal, signal_length, n_streams, d_taps, n_channels, taps_per_channel, power, d_output, hip_stream, 0, 0);
}

int smfft_large_pfb_benchmark(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                              int power, void* d_output, double* FFT_time) {
    const int chk = check(signal_length, n_streams, n_channels, taps_per_channel, 0, 0);
    if (chk != 0) return chk < 0 ? -1 : 0;
    return timed_launch(FFT_time, [&] { return dispatch(d_signal, signal_length, n_streams, d_taps, n_channels, taps_per_channel, power, d_output, 0, 0, nullptr); });
}

}  // extern "C"
#endif

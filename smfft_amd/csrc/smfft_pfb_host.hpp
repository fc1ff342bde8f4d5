// smfft_pfb_host.hpp -- the C ABI half that the two polyphase filter banks share (smfft_pfb.hip, smfft_pfb_real.hip): what is supported,
// the shipped schedule, the checks and the dispatch over the five lengths (the pfb_* functions: smfft_pfb_spec.hip's too).  Host code only,
// internal linkage.  A bank is a struct with
//   kSamplesPerElement              samples of the signal per float2 of the plan: 1 (complex samples), 2 (pairs of real samples: the plan
//                                   is in float2 units, and the signal length must be a whole number of them)
//   launch<N>(x, h, y, plan, power, R, cus, stream)      the per-length launcher of its kernels (untyped pointers)
// and its five extern "C" functions forward to PfbApi<Bank>.  All validation happens before any HIP call.
#pragma once
#include "smfft_addon_host.hpp"
#include "smfft_pfb.hpp"

namespace {
inline bool pfb_supported(int N, int P) { return (N == 256 || N == 512 || N == 1024 || N == 2048 || N == 4096) && P >= 1 && P <= 32; }

template <class Bank>
bool pfb_length_ok(long long L) { return L >= 0 && L % Bank::kSamplesPerElement == 0; }

// the run-time length to the bank's per-length launcher; -1 for a length the banks do not serve
template <class Bank, class... Args>
int pfb_launch_for(int N, const Args&... args) {
    switch (N) {
        case 256: return Bank::template launch<256>(args...);
        case 512: return Bank::template launch<512>(args...);
        case 1024: return Bank::template launch<1024>(args...);
        case 2048: return Bank::template launch<2048>(args...);
        case 4096: return Bank::template launch<4096>(args...);
    }
    return -1;
}

template <class Bank>
struct PfbApi {

    // the shipped run length of the schedule: a starting value, the same for every (N, P) and both banks, until tools/ab_pfb.py and
    // tools/ab_pfb_real.py have been run for it on a device (DESIGN.md sections 12 and 13)
    static int default_tile_run(int N, int P) {
        (void)N;
        (void)P;
        return 4;
    }

    static smfft::PfbPlan plan_of(long long L, int N, int P, int C) { return smfft::PfbPlan{L / Bank::kSamplesPerElement, N, P, C}; }

    // -1: an unsupported combination; 0: launch; 1: nothing to do (no whole frame).  No HIP call.
    static int check(long long L, int C, int N, int P, int tile_run) {
        if (!pfb_supported(N, P) || C <= 0 || !pfb_length_ok<Bank>(L) || tile_run < 0) return -1;
        return plan_of(L, N, P, C).frames() == 0 ? 1 : 0;
    }

    static int dispatch(const void* x, long long L, int C, const void* h, int N, int P, int power, void* y, int tile_run, hipStream_t stream) {
        const int cus = compute_units();
        if (cus <= 0) return (int)hipErrorNoDevice;
        const smfft::PfbPlan plan = plan_of(L, N, P, C);
        const long long R = tile_run > 0 ? tile_run : default_tile_run(N, P);
        return pfb_launch_for<Bank>(N, x, h, y, plan, int(power != 0), R, cus, stream);
    }

    // the bodies of the entry points (*_launch is *_launch_tuned with tile_run = 0)
    static long long frames(long long L, int N, int P) { return pfb_supported(N, P) && pfb_length_ok<Bank>(L) ? plan_of(L, N, P, 1).frames() : -1; }

    static int default_tile_run_or_error(int N, int P) { return pfb_supported(N, P) ? default_tile_run(N, P) : -1; }

    static int launch_tuned(const void* x, long long L, int C, const void* h, int N, int P, int power, void* y, void* hip_stream, int tile_run) {
        const int chk = check(L, C, N, P, tile_run);
        if (chk != 0) return chk < 0 ? -1 : 0;
        return dispatch(x, L, C, h, N, P, power, y, tile_run, (hipStream_t)hip_stream);
    }

    static int benchmark(const void* x, long long L, int C, const void* h, int N, int P, int power, void* y, double* FFT_time) {
        const int chk = check(L, C, N, P, 0);
        if (chk != 0) return chk < 0 ? -1 : 0;
        return timed_launch(FFT_time, [&] { return dispatch(x, L, C, h, N, P, power, y, 0, nullptr); });
    }
};
}  // namespace

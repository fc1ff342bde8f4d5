// smfft_fir_host.hpp -- the C ABI half that the three overlap-save FIR filter banks share (smfft_fir.hip, smfft_fir_real.hip,
// smfft_large_fir.hip): what is supported, the checks, the dispatch over the bank's lengths and the bodies of *_prepare, *_launch and
// *_benchmark.  Host code only, internal linkage.  A bank is a struct with
//   Sizes                                               its lengths, a FirSizes<...>
//   launch<N>(x, w, C, H, K, y, stream)                 the per-length launchers of its kernels (untyped pointers; w: the FirWindow);
//   launch_prepare<N>(taps, M, K, correlate, spectra, stream)      0 or a hipError_t
// and its three extern "C" functions forward to FirApi<Bank>.  All validation happens before any HIP call.
#pragma once
#include <type_traits>

#include "smfft_addon_host.hpp"
#include "smfft_fir.hpp"

namespace {
template <int... Ns>
struct FirSizes {
    static bool has(int N) { return ((N == Ns) || ...); }
    // the run-time length to f(std::integral_constant<int, N>); -1 for a length that is not in the list
    template <class F>
    static int call(int N, F f) {
        int rc = -1;
        (void)((N == Ns && ((rc = f(std::integral_constant<int, Ns>{})), true)) || ...);
        return rc;
    }
};

template <class Bank>
struct FirApi {
    static bool supported(int N) { return Bank::Sizes::has(N); }

    // -1: an unsupported combination; 0: launch; 1: nothing to do (an empty signal).  No HIP call.
    static int check(long long L, int C, int K, int M, int N) {
        if (!supported(N) || M < 1 || M >= N || C <= 0 || K <= 0 || L < 0) return -1;
        return L == 0 ? 1 : 0;
    }

    static int dispatch(const void* x, long long L, int C, const void* H, int K, int M, int N, int correlate, void* y, hipStream_t stream) {
        const smfft::FirWindow w{L, N, M, correlate != 0};
        return Bank::Sizes::call(N, [&](auto n) { return Bank::template launch<decltype(n)::value>(x, w, C, H, K, y, stream); });
    }

    // the bodies of the entry points
    static int prepare(const void* taps, int M, int K, int N, int correlate, void* spectra, void* hip_stream) {
        if (!supported(N) || M < 1 || M >= N || K <= 0) return -1;
        return Bank::Sizes::call(N, [&](auto n) {
            return Bank::template launch_prepare<decltype(n)::value>(taps, M, K, int(correlate != 0), spectra, (hipStream_t)hip_stream);
        });
    }

    static int launch(const void* x, long long L, int C, const void* H, int K, int M, int N, int correlate, void* y, void* hip_stream) {
        const int chk = check(L, C, K, M, N);
        if (chk != 0) return chk < 0 ? -1 : 0;
        return dispatch(x, L, C, H, K, M, N, correlate, y, (hipStream_t)hip_stream);
    }

    static int benchmark(const void* x, long long L, int C, const void* H, int K, int M, int N, int correlate, void* y, double* FFT_time) {
        const int chk = check(L, C, K, M, N);
        if (chk != 0) return chk < 0 ? -1 : 0;
        return timed_launch(FFT_time, [&] { return dispatch(x, L, C, H, K, M, N, correlate, y, nullptr); });
    }
};
}  // namespace

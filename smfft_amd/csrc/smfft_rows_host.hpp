// smfft_rows_host.hpp -- the host layer that the C ABI halves of the eight row libraries share beside smfft_addon_host.hpp
// (smfft_bluestein.hip, smfft_czt.hip, smfft_rowconv.hip, smfft_rowconv_real.hip, smfft_dct.hip, smfft_hilbert.hip, smfft_mdct.hip,
// smfft_stft.hip: rows or frames on ONE register-engine transform of M = 256 ... 4096 points, 4096 / M of them per workgroup): the grid
// rule, the dispatch on M, the interval test and the bodies of the launch / launch_tuned / benchmark entry points.  Host code only, and
// everything has internal linkage.  Each library's check() stays its own: those are the contracts of the headers under include/.
#pragma once
#include <cstdint>
#include <type_traits>

#include "smfft_addon_host.hpp"
#include "smfft_fir_kernel.hpp"

namespace {
constexpr int kGridCap = 12288;     // workgroups along the tiles, grid-strided beyond
static_assert(kGridCap == smfft::kFirGridCap, "the row libraries launch under the cap of the kernels' own header");

// grid <= 0: the default, min(tiles, kGridCap)
int default_grid(int M, long long rows, int grid) {
    if (grid > 0) return grid;
    const long long tiles = (rows + 4096 / M - 1) / (4096 / M);
    return (int)(tiles < kGridCap ? tiles : kGridCap);
}

// M = n / 2 for n a power of two in 512 ... 8192; -1 otherwise
int half_length_fft_size(int n) {
    if (n < 512 || n > 8192 || (n & (n - 1)) != 0) return -1;
    return n / 2;
}

// do [a, a + na elements) and [b, b + nb elements) share a byte
bool overlap(const void* a, unsigned long long na, const void* b, unsigned long long nb, unsigned long long elem_bytes = sizeof(float)) {
    const std::uintptr_t pa = (std::uintptr_t)a, pb = (std::uintptr_t)b;
    return pa < pb ? pb - pa < na * elem_bytes : pa - pb < nb * elem_bytes;
}

// f(std::integral_constant<int, M>{}) for the five lengths; -1 otherwise
template <class F>
int dispatch_m(int M, F f) {
    switch (M) {
        case 256: return f(std::integral_constant<int, 256>{});
        case 512: return f(std::integral_constant<int, 512>{});
        case 1024: return f(std::integral_constant<int, 1024>{});
        case 2048: return f(std::integral_constant<int, 2048>{});
        case 4096: return f(std::integral_constant<int, 4096>{});
    }
    return -1;
}

// The bodies of an entry point triple.  chk: its check()'s verdict (-1: refused; 0: launch; 1: nothing to do); enqueue(grid, stream): the
// launch of `grid` workgroups (<= 0: the default) on `stream`, 0 or the launch's status.
template <class Enqueue>
int checked_launch(int chk, Enqueue enqueue, void* hip_stream) {
    if (chk != 0) return chk < 0 ? -1 : 0;
    return enqueue(0, (hipStream_t)hip_stream);
}

template <class Enqueue>
int checked_launch_tuned(int chk, Enqueue enqueue, void* hip_stream, int grid) {
    if (chk < 0 || grid < 1) return -1;
    if (chk != 0) return 0;
    return enqueue(grid, (hipStream_t)hip_stream);
}

template <class Enqueue>
int checked_benchmark(int chk, Enqueue enqueue, double* FFT_time) {
    if (chk != 0) return chk < 0 ? -1 : 0;
    return timed_launch(FFT_time, [&] { return enqueue(0, nullptr); });
}
}  // namespace

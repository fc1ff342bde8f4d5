// smfft_czt_tables.hpp -- the plan of libsmfft_czt.so (include/smfft_czt.h): the input chirp A, the output chirp C and the spectrum B of
// the convolution kernel b, computed in fp64 and rounded ONCE to fp32, so that the tables' own rounding is the only error they bring to
// every transform.  Plain C++: no HIP, nothing of the device; smfft_czt.hip's C ABI half includes it, and tests/test_sm_czt_cpu.py
// compiles it alone with g++ and the address and undefined-behaviour sanitizers.  The fp64 transform is smfft_bluestein_tables.hpp's.
#pragma once
#include <cmath>
#include <complex>
#include <vector>

#include "smfft_bluestein_tables.hpp"

namespace smfft {
namespace czt {

constexpr int kMaxLength = 2048;

// M: the smallest of 256 ... 4096 with M >= n + m - 1; -1 for n or m outside 1 ... kMaxLength
inline int fft_size(int n, int m) {
    if (n < 1 || n > kMaxLength || m < 1 || m > kMaxLength) return -1;
    int M = 256;
    while (M < n + m - 1) M *= 2;
    return M;
}

// (s q) mod 1 in [-1/2, 1/2], in cycles: the product's rounding error is recovered with one fma and added after the reduction, so the
// result is good to an ulp of 1/2 however large s q is.  q is an integer or half of one.
inline double cycles(double s, double q) {
    const double hi = s * q, lo = std::fma(s, q, -hi);
    return std::remainder(std::remainder(hi, 1.0) + lo, 1.0);
}

// exp(2 pi i p) of a phase p in cycles, |p| <= 3/2: reduced once more, so the angle never leaves [-pi, pi]
inline std::complex<double> unit(double p) {
    const double angle = 2.0 * std::acos(-1.0) * std::remainder(p, 1.0);
    return std::complex<double>(std::cos(angle), std::sin(angle));
}

// the plan of (n, m, start, step) into plan[0, 6M) floats: A[0, M), then B[0, M), then C[0, M), interleaved re, im.  n and m must lie
// in 1 ... kMaxLength, start and step must be finite.
//   A[j] = exp(-2 pi i (j start + step j^2 / 2)), j < n; zero beyond
//   B    = DFT_M(b) / M,  b[t mod M] = exp(+2 pi i step t^2 / 2) for -(n - 1) <= t <= m - 1, zero elsewhere
//   C[k] = exp(-2 pi i step k^2 / 2), k < m; zero beyond
// start is reduced to [-1/2, 1/2] and step to [-1, 1] first (std::remainder: exact).  j is an integer, so a whole cycle of start changes
// no A[j]; j^2 / 2, t^2 / 2 and k^2 / 2 are halves of integers, so two whole cycles of step change no entry of any table.
inline void build_tables(int n, int m, double start, double step, float* plan) {
    const int M = fft_size(n, m);
    start = std::remainder(start, 1.0);
    step = std::remainder(step, 2.0);
    std::vector<std::complex<double>> b((size_t)M, std::complex<double>(0.0, 0.0));
    for (int t = 0; t < m; ++t) b[(size_t)t] = unit(cycles(step, 0.5 * (double)t * (double)t));
    for (int t = 1; t < n; ++t) b[(size_t)(M - t)] = unit(cycles(step, 0.5 * (double)t * (double)t));
    smfft::bluestein::fft64(b);
    for (int j = 0; j < M; ++j) {
        const std::complex<double> zero(0.0, 0.0);
        const double chirp = cycles(step, 0.5 * (double)j * (double)j);
        const std::complex<double> aj = j < n ? unit(-(cycles(start, (double)j) + chirp)) : zero;
        const std::complex<double> cj = j < m ? unit(-chirp) : zero;
        plan[2 * j] = (float)aj.real();
        plan[2 * j + 1] = (float)aj.imag();
        plan[2 * M + 2 * j] = (float)(b[(size_t)j].real() / (double)M);
        plan[2 * M + 2 * j + 1] = (float)(b[(size_t)j].imag() / (double)M);
        plan[4 * M + 2 * j] = (float)cj.real();
        plan[4 * M + 2 * j + 1] = (float)cj.imag();
    }
}

}  // namespace czt
}  // namespace smfft

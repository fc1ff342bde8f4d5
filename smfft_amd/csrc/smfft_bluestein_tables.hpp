// smfft_bluestein_tables.hpp -- the plan of libsmfft_bluestein.so (include/smfft_bluestein.h): the chirp W and the spectrum B of its
// mirror image, computed in fp64 and rounded ONCE to fp32, so that the tables' own rounding is the only error they bring to every
// transform.  Plain C++: no HIP, nothing of the device; smfft_bluestein.hip's C ABI half includes it, and
// tests/test_sm_bluestein_cpu.py compiles it alone with g++ and the address and undefined-behaviour sanitizers.
#pragma once
#include <cmath>
#include <complex>
#include <utility>
#include <vector>

namespace smfft {
namespace bluestein {

constexpr int kMaxLength = 2048;

// M: the smallest of 256 ... 4096 with M >= 2n - 1; -1 for n outside 1 ... kMaxLength
inline int fft_size(int n) {
    if (n < 1 || n > kMaxLength) return -1;
    int M = 256;
    while (M < 2 * n - 1) M *= 2;
    return M;
}

// in-place forward DFT of a.size() = 2^k points in fp64: radix 2, decimation in time, every twiddle from cos / sin of its own angle
inline void fft64(std::vector<std::complex<double>>& a) {
    const size_t M = a.size();
    for (size_t i = 1, j = 0; i < M; ++i) {
        size_t bit = M >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(a[i], a[j]);
    }
    const double pi = std::acos(-1.0);
    std::vector<std::complex<double>> w(M / 2 + 1);
    for (size_t k = 0; k < M / 2; ++k) w[k] = std::complex<double>(std::cos(2.0 * pi * (double)k / (double)M), -std::sin(2.0 * pi * (double)k / (double)M));
    for (size_t len = 2; len <= M; len <<= 1) {
        const size_t half = len / 2, step = M / len;
        for (size_t i = 0; i < M; i += len) {
            for (size_t k = 0; k < half; ++k) {
                const std::complex<double> u = a[i + k], v = a[i + k + half] * w[k * step];
                a[i + k] = u + v;
                a[i + k + half] = u - v;
            }
        }
    }
}

// the plan of (n, inverse) into plan[0, 4M) floats: W[0, M) then B[0, M), interleaved re, im.  n must lie in 1 ... kMaxLength.
//   W[j] = exp(-+ i pi (j^2 mod 2n) / n), j < n; zero beyond            (- forward, + inverse)
//   B    = DFT_M(b) / M,  b[j] = conj(W[j]) (j < n),  b[M - j] = b[j] (1 <= j < n),  zero elsewhere
// b is even, so B is: the upper half is written as the copy of the lower, which makes B[j] == B[M - j] hold to the bit.
inline void build_tables(int n, bool inverse, float* plan) {
    const int M = fft_size(n);
    const double pi = std::acos(-1.0);
    std::vector<std::complex<double>> w((size_t)n), b((size_t)M, std::complex<double>(0.0, 0.0));
    for (int j = 0; j < n; ++j) {
        const long long m = ((long long)j * j) % (2LL * n);          // j^2 mod 2n in integers: the angle never leaves [0, 2 pi)
        const double angle = pi * (double)m / (double)n;
        w[(size_t)j] = std::complex<double>(std::cos(angle), inverse ? std::sin(angle) : -std::sin(angle));
    }
    for (int j = 0; j < n; ++j) {
        b[(size_t)j] = std::conj(w[(size_t)j]);
        if (j > 0) b[(size_t)(M - j)] = b[(size_t)j];
    }
    fft64(b);
    for (int j = 1; j < M / 2; ++j) b[(size_t)(M - j)] = b[(size_t)j];
    for (int j = 0; j < M; ++j) {
        const std::complex<double> wj = j < n ? w[(size_t)j] : std::complex<double>(0.0, 0.0);
        plan[2 * j] = (float)wj.real();
        plan[2 * j + 1] = (float)wj.imag();
        plan[2 * M + 2 * j] = (float)(b[(size_t)j].real() / (double)M);
        plan[2 * M + 2 * j + 1] = (float)(b[(size_t)j].imag() / (double)M);
    }
}

}  // namespace bluestein
}  // namespace smfft

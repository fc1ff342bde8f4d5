// smfft_rowconv_real_scale.hpp -- the integer rule by which libsmfft_rowconv_real.so (include/smfft_rowconv_real.h) balances the two
// real rows it packs into the lanes of one complex transform: from a row's largest magnitude and the fp32 sum of its squares, the
// power of two that brings the row's energy into [1, 4).  Plain C++ and integer arithmetic on the bits of a float: no HIP, nothing of
// the device, no libm; rowconv_real_kernel (smfft_rowconv_real.hip) calls it as a __host__ __device__ function, and
// tests/test_sm_rowconv_real_cpu.py compiles it alone with the host compiler and the address and undefined-behaviour sanitizers, so
// the test reads the very code the kernel runs.  tools/rowconv_real_model.py `row_exponent` is the same rule in NumPy.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMFFT_ROWCONV_REAL_HD __host__ __device__
#else
#define SMFFT_ROWCONV_REAL_HD
#endif

namespace smfft {
namespace rowconv_real {

struct RowScale {
    int k;          // the row enters the transform as ldexp(x, k)
    int zero;       // the row is all zero: every output of its pair is +0 (or NaN, where the partner is not finite)
    int finite;     // 0: the row holds an Inf or a NaN, and every output of its pair is NaN
};

constexpr unsigned kAbsMask = 0x7fffffffu, kInfBits = 0x7f800000u;

// ilogb of the positive finite float with the bits `b` (sign bit clear, b != 0): the exponent of its leading one, -149 ... 127
SMFFT_ROWCONV_REAL_HD inline int ilogb_of_bits(unsigned b) {
    if (b >> 23) return (int)(b >> 23) - 127;
    int top = 22;                                   // a subnormal: the mantissa's leading one counts from 2^-149
    while (!((b >> top) & 1u)) --top;
    return top - 149;
}

// p = ilogb(max |x|) of a row whose largest magnitude has the bits max_bits (the sign bit is ignored); 0 for a row of zeros and for
// one that is not finite, whose squares are never used
SMFFT_ROWCONV_REAL_HD inline int max_exponent(unsigned max_bits) {
    const unsigned b = max_bits & kAbsMask;
    return (b == 0u || b >= kInfBits) ? 0 : ilogb_of_bits(b);
}

// max_bits: the bits of max |x| over the row; s_bits: the bits of s = sum_j ldexp(x_j, -p)^2 in fp32 with p = max_exponent(max_bits),
// which lies in [1, 4 n) for a finite row that is not zero.  k = -p - floor(ilogb(s) / 2): ldexp(x, k) has the energy
// s 2^(-2 floor(ilogb(s) / 2)) in [1, 4).  s is not looked at where the row is zero or not finite: k = 0 there.
SMFFT_ROWCONV_REAL_HD inline RowScale row_scale(unsigned max_bits, unsigned s_bits) {
    const unsigned b = max_bits & kAbsMask, s = s_bits & kAbsMask;
    if (b == 0u) return RowScale{0, 1, 1};
    if (b >= kInfBits) return RowScale{0, 0, 0};
    const int e = (s == 0u || s >= kInfBits) ? 0 : ilogb_of_bits(s);      // (a sum outside its range cannot happen; it shifts nothing)
    return RowScale{-ilogb_of_bits(b) - (e >> 1), 0, 1};                    // >> of a negative e rounds down, as floor does
}

}  // namespace rowconv_real
}  // namespace smfft

// smfft_rows.hpp -- the device pieces that the "real row on ONE half-length complex transform" libraries share (smfft_dct.hip,
// smfft_hilbert.hip, smfft_mdct.hip, smfft_stft.hip: rows of n = 512 ... 8192 floats on the register engine at M = n / 2): the first
// octant of W_32768 and its extension by symmetry, the read of a twiddle row's entry, the per-tile value and the row accesses with their
// cache policy as a template argument.  Included by the per-length halves of those files (behind smfft_fir_kernel.hpp).
//
// Everything here is used at compile time or inlined: no kernel, no __device__ object.  Each library keeps its kernels, its
// launch_*<M> and its Rows<M> / rows<M> in its own namespace -- the Rows structs differ (wn; wn, w4; pre, post) and the kernels name
// the objects by symbol -- and its SMFFT_<LIB>_NT_* macros, which it hands to the accesses below in one-line wrappers.  The partner
// exchange through LDS (sf[u + T q] = r[q] ... partner[T (15 - q)]) stays in the kernels: where its barriers stand differs between
// them.
#pragma once
#include <hip/hip_runtime.h>

#include "smfft/smfft_engine.hpp"

namespace smfft {
namespace rows {

static constexpr TwiddleValue octant_32768[4097] = {
#include "smfft/smfft_twiddles_dct.inc"
};

// (cos, sin)(2 pi m / 32768), 0 <= m < 16384, from the octant: exact symmetries, so every entry is an fp64 value rounded once
constexpr TwiddleValue w32768(int m) {
    const int q = m / 4096, r = m % 4096;
    const TwiddleValue a = octant_32768[r], b = octant_32768[4096 - r];
    return q == 0 ? TwiddleValue{a.x, a.y} : q == 1 ? TwiddleValue{b.y, b.x} : q == 2 ? TwiddleValue{-a.y, a.x} : TwiddleValue{-b.x, b.y};
}

__device__ __forceinline__ float2 row_entry(const TwiddleValue* p) {
    const TwiddleValue v = *p;
    return make_float2(v.x, v.y);
}

// v, as a value the compiler takes for new in every tile: the twiddle loads indexed with it stay inside the tile loop, where their
// registers are free again behind the use, and are not kept across the loop (thirty-two to forty-eight float2 per thread: with them
// resident the kernels need more than 256 VGPRs, one wave per SIMD)
__device__ __forceinline__ int per_tile(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

// two or four consecutive floats of a row at 4-byte alignment (the rows' contract), and one complex value at 8-byte alignment
typedef float row_pair __attribute__((ext_vector_type(2), aligned(4)));
typedef float row_quad __attribute__((ext_vector_type(4), aligned(4)));
typedef float bin_pair __attribute__((ext_vector_type(2)));

// one, two or four consecutive floats, or one complex value, of global memory; NT: true non-temporal, false plain.  (Each spells
// its access out: a helper templated on the vector type would deduce it without its alignment.)
template <bool NT>
__device__ __forceinline__ float gload1(const float* p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}
template <bool NT>
__device__ __forceinline__ float2 gload2(const float* p) {
    row_pair v;
    if constexpr (NT) v = __builtin_nontemporal_load(reinterpret_cast<const row_pair*>(p));
    else v = *reinterpret_cast<const row_pair*>(p);
    return make_float2(v.x, v.y);
}
template <bool NT>
__device__ __forceinline__ row_quad gload4(const float* p) {
    if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const row_quad*>(p));
    else return *reinterpret_cast<const row_quad*>(p);
}
template <bool NT>
__device__ __forceinline__ float2 gloadc(const float2* p) {
    bin_pair v;
    if constexpr (NT) v = __builtin_nontemporal_load(reinterpret_cast<const bin_pair*>(p));
    else v = *reinterpret_cast<const bin_pair*>(p);
    return make_float2(v.x, v.y);
}
template <bool NT>
__device__ __forceinline__ void gstore1(float* p, float v) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}
template <bool NT>
__device__ __forceinline__ void gstore2(float* p, float a, float b) {
    const row_pair v = {a, b};
    if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<row_pair*>(p));
    else *reinterpret_cast<row_pair*>(p) = v;
}
template <bool NT>
__device__ __forceinline__ void gstore4(float* p, row_quad v) {
    if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<row_quad*>(p));
    else *reinterpret_cast<row_quad*>(p) = v;
}
template <bool NT>
__device__ __forceinline__ void gstorec(float2* p, float a, float b) {
    const bin_pair v = {a, b};
    if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<bin_pair*>(p));
    else *reinterpret_cast<bin_pair*>(p) = v;
}

}  // namespace rows
}  // namespace smfft

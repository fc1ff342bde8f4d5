// smfft_fir_kernel.hpp -- what the kernels of the overlap-save FIR filter banks at N = 256 ... 4096 share (smfft_fir.hip: complex data,
// smfft_fir_real.hip: real signals and real taps): the launch constants and the launcher pair.  The C ABI halves share
// smfft_fir_host.hpp.  (The banks at N = 8192 / 16384 are another engine with another work split: include/smfft/smfft_large_fir.hpp.)
//
// The kernel bodies are NOT shared, although fir_real_overlap_save_kernel is fir_overlap_save_kernel with another unit, load and
// store.  A __device__ __forceinline__ fir_body<N, Bank> called from both __global__ wrappers was written and compiled: hipcc simplifies
// such a body once on its own and once more inside the wrapper, and all twenty kernels come out different from the ones that were
// measured and are documented (the complex kernel at N = 256: 1838 -> 1825 instructions with other compare and select forms; the
// prepare kernels: other operand orders and instruction counts), with or without __restrict__ on the body's parameters.  The bank is
// not what changes them: fir_overlap_save_kernel's own statements, moved unchanged behind one forceinline function, compile to the
// same other code.  With the statements in the kernel itself the code is what it was, so that is where they stay.
#pragma once
#include <hip/hip_runtime.h>

#include "smfft/smfft_engine.hpp"
#include "smfft_fir.hpp"

namespace smfft {

constexpr int kFirThreads = 256;
constexpr int kFirGridCap = 12288;          // workgroups along the unit tiles (grid-strided beyond), as the external kernels
constexpr int kFirTargetWorkgroups = 2048;  // the filter-group rule's target: twice the workgroups the chip holds at once

// enqueue a bank's kernels on `stream`; units: the plan's segments (complex) or pairs of segments (real) per channel; 0 or the launch's
// hipError_t
template <int N, class Kernel, class Sample, class Plan>
int fir_launch(Kernel kernel, const Sample* x, const Plan& plan, long long units, int C, const float2* H, int K, Sample* y, hipStream_t stream) {
    const long long tiles = (units * C + Geometry<N>::kFftsPerBlock - 1) / Geometry<N>::kFftsPerBlock;
    const int group = fir_filter_group_size(tiles, K, kFirTargetWorkgroups);
    const dim3 grid((unsigned)(tiles < kFirGridCap ? tiles : kFirGridCap), (unsigned)((K + group - 1) / group));
    hipLaunchKernelGGL(kernel, grid, dim3(kFirThreads), 0, stream, x, H, y, plan, C, K, group);
    return (int)hipGetLastError();
}

template <int N, class Kernel, class Tap>
int fir_launch_prepare(Kernel kernel, const Tap* taps, int M, int K, int correlate, float2* spectra, hipStream_t stream) {
    constexpr int F = Geometry<N>::kFftsPerBlock;
    hipLaunchKernelGGL(kernel, dim3((K + F - 1) / F), dim3(kFirThreads), 0, stream, taps, M, K, correlate, spectra);
    return (int)hipGetLastError();
}

}  // namespace smfft

// smfft_fir.hpp -- the segmentation of the overlap-save FIR filter banks (smfft_fir.hip, include/smfft.h "FIR filter banks"), in one
// place for the host launch, the kernel and the CPU test that compiles it against tools/fir_plan_model.py.
//
// A channel x[0, L) is cut into S = ceil(L / V) segments of N samples, V = N - M + 1.  Segment s is the N samples x[a(s) + e], e < N,
// read as zero outside [0, L), with
//     a(s) = s V - (M - 1)      convolve:  y[n] = sum_m h[m] x[n - m]
//     a(s) = s V                correlate: y[n] = sum_m conj(h[m]) x[n + m]
// Its circular convolution with g (g = h, or g[m] = conj(h[M-1-m]) for correlate: the prepared spectrum is DFT_N(pad_N(g)) / N) equals
// the linear one at the elements j >= M - 1, whichever the mode: element j of segment s is output
//     n = s V + j - (M - 1),    stored if  M - 1 <= j < N  and  n < L,
// so the segments' stored windows tile [0, L) exactly once.  The two modes differ in the load start alone (correlation is convolution
// with g, whose output is M - 1 samples late).
#pragma once
#include <hip/hip_runtime.h>

namespace smfft {

struct FirWindow {
    long long L;   // samples per channel (>= 1)
    int N, M;      // transform length, taps (1 <= M <= N - 1)
    int correlate; // 0: convolve, 1: correlate

    __host__ __device__ int valid() const { return N - M + 1; }                                       // V: outputs per segment
    __host__ __device__ long long segments() const { return (L + valid() - 1) / valid(); }            // S
    __host__ __device__ long long load_start(long long s) const { return s * valid() - (correlate ? 0 : M - 1); }
    // store window of segment s: elements j in [store_begin, store_end(s))
    __host__ __device__ int store_begin() const { return M - 1; }
    __host__ __device__ int store_end(long long s) const {
        const long long left = L - s * valid() + (M - 1);     // first j whose output would be n >= L
        return left < N ? (int)left : N;
    }
    // output sample of element j of segment s (the offset inside the (channel, filter) row of length L)
    __host__ __device__ long long output_index(long long s, int j) const { return s * valid() + j - (M - 1); }
};

// The filter-group rule: a launch over `tiles` workgroup tiles (4096 / N segments each) splits its K filters into groups -- one more
// grid row each, every group recomputing its segments' forward transforms -- until tiles x groups reaches `target` workgroups or every
// group holds one filter: groups = min(K, ceil(target / tiles)), and the group size is ceil(K / groups).
__host__ __device__ inline int fir_filter_group_size(long long tiles, int K, int target) {
    long long groups = (target + tiles - 1) / tiles;
    if (groups > K) groups = K;
    if (groups < 1) groups = 1;
    return (int)((K + groups - 1) / groups);
}

}  // namespace smfft

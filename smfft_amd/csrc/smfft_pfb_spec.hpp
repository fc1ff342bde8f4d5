// smfft_pfb_spec.hpp -- the index arithmetic of the integrated power spectra of the polyphase filter banks (smfft_pfb_spec.hip,
// include/smfft_pfb_spec.h), in one place for the host launch, the kernel and the CPU test that compiles it against
// tools/pfb_spec_model.py.  Units are those of smfft_pfb.hpp: float2 elements, one complex sample or two real ones, so a frame is N
// elements in both banks.
//
// C streams of L elements, a prototype of P taps per channel, hop N: F = floor(L / N) - P + 1 frames per stream (0 if that is not
// positive), as PfbPlan has them.  T consecutive frames are integrated into one spectrum: I = floor(F / T) spectra per stream; the
// F - I T trailing frames are not computed and their samples, beyond element (I T + P - 1) N of a stream, are not read.
//
// The C I (stream, spectrum) groups are numbered g = c I + i and cut into tiles of 4096 / N consecutive groups -- one workgroup's worth;
// a tile may straddle streams, the last one may be partial.  Frame t < T of group g reads P N elements from element
// c L + (i T + t) N of the signal; the group writes N floats to element g N of the output (the output IS group-major).  Workgroup b of a
// grid of G takes the tiles b, b + G, ...  Which tile a group is computed in does not enter its arithmetic.
#pragma once
#include <hip/hip_runtime.h>

namespace smfft {

struct PfbSpecPlan {
    long long L;   // elements per stream (>= 0)
    int N, P;      // channels (the transform length), taps per channel
    int C;         // streams
    int T;         // frames per spectrum (>= 1)

    __host__ __device__ long long frames() const {
        const long long f = L / N - P + 1;
        return f > 0 ? f : 0;
    }
    __host__ __device__ long long spectra() const { return frames() / T; }
    __host__ __device__ long long groups() const { return spectra() * C; }
    __host__ __device__ int per_tile() const { return 4096 / N; }
    __host__ __device__ long long tiles() const { return (groups() + per_tile() - 1) / per_tile(); }
    // the group of slot j of a tile, or -1 for a slot beyond the last group (a partial last tile)
    __host__ __device__ long long group_of(long long tile, int j) const {
        const long long g = tile * per_tile() + j;
        return g < groups() ? g : -1;
    }
    __host__ __device__ long long stream_of(long long g) const { return g / spectra(); }
    __host__ __device__ long long spectrum_of(long long g) const { return g % spectra(); }
    // first signal element of the window of frame t of group g (tap p, channel phase n: + p N + n), first output element of its spectrum
    __host__ __device__ long long input_offset(long long g, long long t) const { return stream_of(g) * L + (spectrum_of(g) * T + t) * N; }
    __host__ __device__ long long output_offset(long long g) const { return g * N; }
    // elements of a stream that a launch reads: [0, used())
    __host__ __device__ long long used() const { return spectra() > 0 ? (spectra() * T + P - 1) * N : 0; }
    // the persistent grid (needs tiles() >= 1)
    __host__ __device__ long long grid(long long max_workgroups) const {
        const long long n = tiles();
        return n < max_workgroups ? n : max_workgroups;
    }
};

}  // namespace smfft

// smfft_pfb.hpp -- the index arithmetic of the polyphase filter bank channelizer (smfft_pfb.hip, include/smfft_pfb.h), in one place for
// the host launch, the kernel and the CPU test that compiles it against tools/pfb_model.py.
//
// C streams of L samples, a prototype of P N real taps, hop N.  A stream holds F = floor(L / N) - P + 1 output frames (0 if that is not
// positive); frame f of stream c is the N-point transform of
//     w[n] = sum_{p<P} h[p N + n] x_c[(f + p) N + n],
// so it reads x_c[f N, (f + P) N) and nothing beyond (F + P - 1) N <= L: every frame is whole, there is no zero fill.
//
// The C F (stream, frame) pairs are numbered g = c F + f and cut into tiles of 4096 / N consecutive pairs -- one workgroup's worth; a
// tile may straddle streams, the last one may be partial.  Pair g reads from element c L + f N of the signal and writes to element g N
// of the output (the output IS pair-major).
//
// The schedule: the tiles are cut into runs of R consecutive tiles, run j = tiles [j R, min((j + 1) R, tiles)), and workgroup b of a
// grid of G takes the runs j = b, b + G, ...  R = 1 is the plain grid-stride loop; a larger R gives a workgroup neighbouring tiles,
// whose windows overlap in P - 1 of their frames.  Which tile a pair is computed in does not enter its arithmetic.
#pragma once
#include <hip/hip_runtime.h>

namespace smfft {

struct PfbPlan {
    long long L;   // samples per stream (>= 0)
    int N, P;      // channels (the transform length), taps per channel
    int C;         // streams

    __host__ __device__ long long frames() const {
        const long long f = L / N - P + 1;
        return f > 0 ? f : 0;
    }
    __host__ __device__ long long pairs() const { return frames() * C; }
    __host__ __device__ int per_tile() const { return 4096 / N; }
    __host__ __device__ long long tiles() const { return (pairs() + per_tile() - 1) / per_tile(); }
    // the pair of slot j of a tile, or -1 for a slot beyond the last pair (a partial last tile)
    __host__ __device__ long long pair_of(long long tile, int j) const {
        const long long g = tile * per_tile() + j;
        return g < pairs() ? g : -1;
    }
    __host__ __device__ long long stream_of(long long g) const { return g / frames(); }
    __host__ __device__ long long frame_of(long long g) const { return g % frames(); }
    // first signal element of pair g's window (tap p, channel phase n: + p N + n), first output element of its spectrum
    __host__ __device__ long long input_offset(long long g) const { return stream_of(g) * L + frame_of(g) * N; }
    __host__ __device__ long long output_offset(long long g) const { return g * N; }

    // the schedule (needs tiles() >= 1)
    __host__ __device__ long long run_length(long long R) const {
        const long long t = tiles();
        return R < 1 ? 1 : (R > t ? t : R);
    }
    __host__ __device__ long long runs(long long R) const {
        const long long r = run_length(R);
        return (tiles() + r - 1) / r;
    }
    __host__ __device__ long long grid(long long max_workgroups, long long R) const {
        const long long n = runs(R);
        return n < max_workgroups ? n : max_workgroups;
    }
    __host__ __device__ long long run_begin(long long j, long long R) const { return j * run_length(R); }
    __host__ __device__ long long run_end(long long j, long long R) const {
        const long long e = (j + 1) * run_length(R), t = tiles();
        return e < t ? e : t;
    }
};

}  // namespace smfft

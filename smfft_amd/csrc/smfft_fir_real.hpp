// smfft_fir_real.hpp -- the pairing of the overlap-save FIR filter banks for real signals and real taps (smfft_fir_real.hip,
// include/smfft_fir_real.h), in one place for the host launch, the kernel and the CPU test that compiles it against
// tools/fir_real_model.py.
//
// The segmentation is smfft_fir.hpp's FirWindow, unchanged.  For a real filter g, conv(x1 + i x2, g) = conv(x1, g) + i conv(x2, g), so
// two consecutive segments of one channel ride in the real and the imaginary lane of one complex transform: a channel of S segments
// is P = ceil(S / 2) pairs, pair p = segments 2p (lane 0, `.x`) and 2p + 1 (lane 1, `.y`).  The last pair of a channel with an odd S
// has no second segment: its `.y` is loaded as zero and never stored.  A pair never spans two channels.
#pragma once
#include "smfft_fir.hpp"

namespace smfft {

struct FirPairs {
    FirWindow w;

    __host__ __device__ long long pairs() const { return (w.segments() + 1) / 2; }                      // P, per channel
    __host__ __device__ long long segment(long long p, int lane) const { return 2 * p + lane; }
    __host__ __device__ bool present(long long p, int lane) const { return segment(p, lane) < w.segments(); }
    // lane `lane` of register element e of pair p is x[load_start(p, lane) + e], zero outside [0, L) and zero when the segment is absent
    __host__ __device__ long long load_start(long long p, int lane) const { return w.load_start(segment(p, lane)); }
    // store window of a lane: elements j in [w.store_begin(), store_end(p, lane)), empty for an absent segment
    __host__ __device__ int store_end(long long p, int lane) const { return present(p, lane) ? w.store_end(segment(p, lane)) : 0; }
    // output sample of element j of a lane (the offset inside the (channel, filter) row of length L)
    __host__ __device__ long long output_index(long long p, int lane, int j) const { return w.output_index(segment(p, lane), j); }
};

}  // namespace smfft

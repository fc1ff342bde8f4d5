/*
 * smfft_large_pfb.h -- C ABI of libsmfft_large_pfb.so: the critically sampled polyphase filter bank (PFB) channelizer of smfft_pfb.h for
 * N = 8192 and 16384 channels -- a prototype low-pass of P*N real taps applied to a long complex stream and an N-point forward FFT
 * across its P polyphase branches -- in one kernel from signal load to spectrum store, on the single-pass engine of smfft_large.h
 * (include/smfft/smfft_large_pfb.hpp, smfft_amd/csrc/smfft_large_pfb.hip).
 *
 * Definition (that of smfft_pfb.h):
 *   - signal d_signal: C streams x L float2, stream c at element c*L (L = signal_length, any value >= 0, 64-bit offsets);
 *   - prototype d_taps: P*N REAL fp32 coefficients, h[p*N + n], shared by all streams (N = n_channels, P = taps_per_channel);
 *   - frames per stream F = floor(L / N) - P + 1 (0 if that is not positive).  Samples beyond (F + P - 1)*N of a stream are never
 *     read; no sample outside [0, C*L) is read at all (every frame is whole, so there is no zero fill);
 *   - output d_output, complex mode: C*F*N float2,
 *
 *         y[(c*F + f)*N + k] = sum_{n<N} ( sum_{p<P} h[p*N + n] * x_c[(f + p)*N + n] ) * exp(-2 pi i n k / N)
 *
 *     natural channel order, un-normalised, the forward sign of smfft_large_launch;
 *   - power mode (power != 0): C*F*N float, |y|^2 of the above;
 *   - N in {8192, 16384}; 1 <= P <= 32;
 *   - buffer contract: pointers 8-byte aligned (4 for taps and the power output), interior pointers are fine; signal, taps and output
 *     must not overlap; every output element is written exactly once; no workspace and no allocation inside a call, so a launch can
 *     be captured into a graph.
 * Return values: 0, a hipError_t, or -1 -- before any HIP call -- for an unsupported combination (n_channels, taps_per_channel,
 * n_streams <= 0, signal_length < 0, schedule < 0 or > 2, max_workgroups < 0).  F == 0 launches nothing and returns 0.
 *
 * Out of scope: N <= 4096 (that is smfft_pfb.h: libsmfft_pfb.so), real-valued input, oversampled banks (hop != N), complex prototypes,
 * the synthesis (inverse) bank.
 */
#ifndef SMFFT_LARGE_PFB_H_
#define SMFFT_LARGE_PFB_H_

#ifdef __cplusplus
extern "C" {
#endif

/* F for one stream of signal_length samples, or -1 for an unsupported n_channels / taps_per_channel or signal_length < 0.  No HIP
 * call. */
long long smfft_large_pfb_frames(long long signal_length, int n_channels, int taps_per_channel);

/* Channelizes n_streams streams, enqueued on hip_stream (a hipStream_t; NULL = the null stream).  Launch only: no synchronisation. */
int smfft_large_pfb_launch(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                           int power, void* d_output, void* hip_stream);

/* The same launch on the null stream, timed with events: ADDS the elapsed milliseconds to *FFT_time (when the launch was made and
 * FFT_time is not NULL) and returns after the kernel has finished. */
int smfft_large_pfb_benchmark(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                              int power, void* d_output, double* FFT_time);

/* Tuning and tests only: smfft_large_pfb_launch with the schedule and the grid given by the caller.  One workgroup computes one
 * (stream, frame) pair at a time; in round t workgroup b of a grid of G takes pair t*G + b (schedule 1, stride) or pair
 * t*G + (b mod 8)*(G/8) + b/8 (schedule 2, XCD-blocked: G is rounded down to a multiple of 8, and a grid below 8 falls back to
 * schedule 1).  G = min(pairs, max_workgroups, what the device holds at once).  0 = the shipped default, for either.  The results do
 * not depend on them, to the bit.  Arguments, not process-wide settings: launches on different streams cannot disturb each other. */
int smfft_large_pfb_launch_tuned(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                                 int power, void* d_output, void* hip_stream, int schedule, int max_workgroups);

/* The schedule a plain launch uses (1 or 2); -1 for an unsupported n_channels / taps_per_channel.  No HIP call. */
int smfft_large_pfb_default_schedule(int n_channels, int taps_per_channel);

#ifdef __cplusplus
}
#endif

#endif /* SMFFT_LARGE_PFB_H_ */

/*
 * smfft_pfb.h -- C ABI of libsmfft_pfb.so: the critically sampled polyphase filter bank (PFB) channelizer -- a prototype low-pass of
 * P*N real taps applied to a long complex stream and an N-point forward FFT across its P polyphase branches, N evenly spaced channels
 * per N input samples -- in one kernel from signal load to spectrum store (smfft_amd/csrc/smfft_pfb.hip).
 *
 * Definition:
 *   - signal d_signal: C streams x L float2, stream c at element c*L (L = signal_length, any value >= 0, 64-bit offsets);
 *   - prototype d_taps: P*N REAL fp32 coefficients, h[p*N + n], shared by all streams (N = n_channels, P = taps_per_channel);
 *   - frames per stream F = floor(L / N) - P + 1 (0 if that is not positive).  Samples beyond (F + P - 1)*N of a stream are never
 *     read; no sample outside [0, C*L) is read at all (every frame is whole, so there is no zero fill);
 *   - output d_output, complex mode: C*F*N float2,
 *
 *         y[(c*F + f)*N + k] = sum_{n<N} ( sum_{p<P} h[p*N + n] * x_c[(f + p)*N + n] ) * exp(-2 pi i n k / N)
 *                            = sum_{m<P*N} h[m] * x_c[f*N + m] * exp(-2 pi i k m / N)
 *
 *     natural channel order, un-normalised, the forward sign of smfft_launch;
 *   - power mode (power != 0): C*F*N float, |y|^2 of the above (detection fused into the store: half the output bytes);
 *   - N in {256, 512, 1024, 2048, 4096}; 1 <= P <= 32;
 *   - buffer contract: pointers 8-byte aligned (4 for taps and the power output), interior pointers are fine; signal, taps and output
 *     must not overlap; every output element is written exactly once; no workspace and no allocation inside a call, so a launch can
 *     be captured into a graph.
 * Return values: 0, a hipError_t, or -1 -- before any HIP call -- for an unsupported combination (n_channels, taps_per_channel,
 * n_streams <= 0, signal_length < 0, tile_run < 0).  F == 0 launches nothing and returns 0.
 *
 * Out of scope: oversampled banks (hop != N), real-valued input (that is smfft_pfb_real.h: libsmfft_pfb_real.so), complex prototypes,
 * the synthesis (inverse) bank, N <= 128 (16 or fewer threads per FFT would load 8 ... 64-byte pieces: that needs a staging path of
 * its own, as for smfft_fir_*) and N >= 8192.
 */
#ifndef SMFFT_PFB_H_
#define SMFFT_PFB_H_

#ifdef __cplusplus
extern "C" {
#endif

/* F for one stream of signal_length samples, or -1 for an unsupported n_channels / taps_per_channel or signal_length < 0.  No HIP
 * call. */
long long smfft_pfb_frames(long long signal_length, int n_channels, int taps_per_channel);

/* Channelizes n_streams streams, enqueued on hip_stream (a hipStream_t; NULL = the null stream).  Launch only: no synchronisation. */
int smfft_pfb_launch(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                     int power, void* d_output, void* hip_stream);

/* The same launch on the null stream, timed with events: ADDS the elapsed milliseconds to *FFT_time (when the launch was made and
 * FFT_time is not NULL) and returns after the kernel has finished. */
int smfft_pfb_benchmark(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                        int power, void* d_output, double* FFT_time);

/* Tuning and tests only: smfft_pfb_launch with the schedule's run length given by the caller.  A workgroup takes runs of tile_run
 * consecutive tiles (a tile = 4096 / N consecutive frames); tile_run >= 1, 0 = the shipped default (what smfft_pfb_launch passes).
 * The results do not depend on it, to the bit.  An argument, not a process-wide setting: launches on different streams cannot
 * disturb each other. */
int smfft_pfb_launch_tuned(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                           int power, void* d_output, void* hip_stream, int tile_run);

/* The tile_run a plain launch uses; -1 for an unsupported n_channels / taps_per_channel.  No HIP call. */
int smfft_pfb_default_tile_run(int n_channels, int taps_per_channel);

#ifdef __cplusplus
}
#endif

#endif /* SMFFT_PFB_H_ */

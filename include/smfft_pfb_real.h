/*
 * smfft_pfb_real.h -- C ABI of libsmfft_pfb_real.so: the critically sampled polyphase filter bank (PFB) channelizer for REAL streams --
 * a prototype low-pass of P*2N real taps applied to a long real stream and a 2N-point real-to-complex transform across its P polyphase
 * branches, N channels (0 ... N - 1, plus the Nyquist value packed beside DC) per 2N input samples -- in one kernel from signal load
 * to spectrum store (smfft_amd/csrc/smfft_pfb_real.hip).  The complex bank is smfft_pfb.h; against converting a
 * real stream to complex and running that bank with 2N channels this one reads half the bytes, does half the transform work and
 * writes no redundant half spectrum.
 *
 * Definition:
 *   - signal d_signal: C streams x L FLOAT, stream c at element c*L (L = signal_length >= 0, 64-bit offsets).  L must be EVEN: the
 *     real-array rule of the buffer contract in smfft.h (an even number of floats from an 8-byte-aligned base), which keeps every
 *     stream 8-byte aligned.  An odd L returns -1;
 *   - prototype d_taps: P*2N REAL fp32 coefficients, h[p*2N + n], shared by all streams (N = n_channels, P = taps_per_channel);
 *   - frames per stream F = floor(L / 2N) - P + 1 (0 if that is not positive): frames of 2N real samples, hop 2N.  Samples beyond
 *     (F + P - 1)*2N of a stream are never read; no sample outside [0, C*L) is read at all (every frame is whole, so there is no
 *     zero fill);
 *   - the spectrum of frame f of stream c, for 0 <= k <= N, un-normalised, the forward sign of smfft_launch:
 *
 *         X_f[k] = sum_{n<2N} ( sum_{p<P} h[p*2N + n] * x_c[(f + p)*2N + n] ) * exp(-2 pi i n k / 2N)
 *                = sum_{m<2PN} h[m] * x_c[2fN + m] * exp(-2 pi i k m / 2N)
 *
 *     (X_f[2N - k] = conj(X_f[k]) is not output; X_f[0] and X_f[N] are real);
 *   - output d_output, complex mode: C*F*N float2, pair-major as in the complex bank: y[(c*F + f)*N + k] = X_f[k] for 1 <= k < N, and
 *     element 0 of a row is (Re X_f[0], Re X_f[N]) -- the packed DC / Nyquist layout of smfft_rc_external_benchmark;
 *   - power mode (power != 0): C*F*N float: |X_f[k]|^2 for 1 <= k < N, and element 0 is X_f[0]^2 (DC).  The Nyquist power X_f[N]^2
 *     is NOT output in power mode: a caller that needs it runs the complex mode;
 *   - N in {256, 512, 1024, 2048, 4096}; 1 <= P <= 32;
 *   - buffer contract: signal, taps and the complex output 8-byte aligned (the power output 4), interior pointers at an even number
 *     of floats are fine; signal, taps and output must not overlap; every output element is written exactly once; no workspace and
 *     no allocation inside a call, so a launch can be captured into a graph.
 * Return values: 0, a hipError_t, or -1 -- before any HIP call -- for an unsupported combination (n_channels, taps_per_channel,
 * n_streams <= 0, signal_length < 0 or odd, tile_run < 0).  F == 0 launches nothing and returns 0.
 *
 * Out of scope: oversampled banks (hop != 2N), complex prototypes, the synthesis (inverse) bank, a Nyquist power output, N <= 128 and
 * N >= 8192.
 */
#ifndef SMFFT_PFB_REAL_H_
#define SMFFT_PFB_REAL_H_

#ifdef __cplusplus
extern "C" {
#endif

/* F for one stream of signal_length floats, or -1 for an unsupported n_channels / taps_per_channel or a signal_length that is
 * negative or odd.  No HIP call. */
long long smfft_pfb_real_frames(long long signal_length, int n_channels, int taps_per_channel);

/* Channelizes n_streams streams, enqueued on hip_stream (a hipStream_t; NULL = the null stream).  Launch only: no synchronisation. */
int smfft_pfb_real_launch(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                          int power, void* d_output, void* hip_stream);

/* The same launch on the null stream, timed with events: ADDS the elapsed milliseconds to *FFT_time (when the launch was made and
 * FFT_time is not NULL) and returns after the kernel has finished. */
int smfft_pfb_real_benchmark(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                             int power, void* d_output, double* FFT_time);

/* Tuning and tests only: smfft_pfb_real_launch with the schedule's run length given by the caller.  A workgroup takes runs of
 * tile_run consecutive tiles (a tile = 4096 / N consecutive frames); tile_run >= 1, 0 = the shipped default (what
 * smfft_pfb_real_launch passes).  The results do not depend on it, to the bit.  An argument, not a process-wide setting: launches on
 * different streams cannot disturb each other. */
int smfft_pfb_real_launch_tuned(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                                int power, void* d_output, void* hip_stream, int tile_run);

/* The tile_run a plain launch uses; -1 for an unsupported n_channels / taps_per_channel.  No HIP call. */
int smfft_pfb_real_default_tile_run(int n_channels, int taps_per_channel);

#ifdef __cplusplus
}
#endif

#endif /* SMFFT_PFB_REAL_H_ */

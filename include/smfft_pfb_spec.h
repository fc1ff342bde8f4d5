/*
 * smfft_pfb_spec.h -- C ABI of libsmfft_pfb_spec.so: INTEGRATED POWER SPECTRA of the critically sampled polyphase filter banks of
 * smfft_pfb.h (complex streams: smfft_pfb_spec_*) and smfft_pfb_real.h (real streams: smfft_pfb_real_spec_*).  The kernel is the bank's
 * own -- weighted sum over the P polyphase branches, N-point transform, power -- and sums the power of n_integrate consecutive frames
 * in the thread that computed it, so one spectrum per n_integrate frames goes out instead of one per frame: the spectrometer's
 * accumulation without the stream of per-frame powers and without a reduction pass (smfft_amd/csrc/smfft_pfb_spec.hip, DESIGN.md
 * section 15).
 *
 * Definition (notation of smfft_pfb.h / smfft_pfb_real.h; "frame" = N complex samples, or 2N real samples in the real bank):
 *   - signal d_signal: C streams x L samples (float2, or float in the real bank, where L must be EVEN), stream c at element c*L
 *     (L = signal_length >= 0, 64-bit offsets); prototype d_taps: P*N (real bank: P*2N) REAL fp32 coefficients, shared by all streams;
 *   - F = frames per stream as smfft_pfb_frames / smfft_pfb_real_frames define it; T = n_integrate >= 1; I = floor(F / T) spectra per
 *     stream.  The trailing frames f >= I*T are not computed: samples beyond (I*T + P - 1) frames of a stream are never read, and no
 *     sample outside [0, C*L) is read at all;
 *   - output d_output: C*I*N float, group-major:
 *
 *         S[(c*I + i)*N + k] = sum_{t<T} p[c, i*T + t, k]
 *
 *     where p[c, f, k] is exactly the value the same bank's power mode (power != 0) stores for frame f of stream c: fmaf(re, re, im*im)
 *     in fp32 of the spectrum value it computes.  The real bank keeps its packed convention: channel 0 is the power of X[0] alone, and
 *     the Nyquist power is NOT output;
 *   - the sum runs in fp32 in frame order: acc = p_0, then acc = acc + p_t for t = 1 ... T - 1, every p_t rounded to fp32 before the
 *     add.  With T = 1 the output equals the bank's power mode bit for bit;
 *   - N in {256, 512, 1024, 2048, 4096}; 1 <= P <= 32;
 *   - buffer contract, as the banks': signal 8-byte aligned, taps and output 4-byte aligned (real bank's taps: 8), interior pointers
 *     are fine; signal, taps and output must not overlap; every output element is written exactly once; no workspace, no allocation
 *     and no atomics inside a call, so a launch can be captured into a graph and is deterministic.
 * Return values: 0, a hipError_t, or -1 -- before any HIP call -- for an unsupported combination (n_channels, taps_per_channel,
 * n_integrate <= 0, n_streams <= 0, signal_length < 0, an odd signal_length in the real bank, max_workgroups < 0).  I == 0 launches
 * nothing and returns 0.
 *
 * Out of scope:
 *   - N >= 8192 (smfft_large_pfb.h has the channelizer there, without integration) and N <= 128;
 *   - cross-products between streams (Stokes parameters, correlators): every stream is detected on its own;
 *   - parallelism beyond C*I*N/4096 workgroups: a (stream, spectrum) group is one thread slot's work.  A caller with few streams and a
 *     very long integration integrates a shorter T here and sums the few resulting spectra afterwards;
 *   - the growth of fp32 rounding with T: the sum is sequential, its error bound grows like (T - 1) 2^-24 relative to the sum.  No
 *     compensated or pairwise summation, no fp64 accumulator;
 *   - a Nyquist power output in the real bank, oversampled banks, complex prototypes and the synthesis (inverse) bank, as in the
 *     banks' own headers.
 */
#ifndef SMFFT_PFB_SPEC_H_
#define SMFFT_PFB_SPEC_H_

#ifdef __cplusplus
extern "C" {
#endif

/* I for one stream of signal_length samples, or -1 for an unsupported n_channels / taps_per_channel, n_integrate <= 0 or a negative
 * (real bank: or odd) signal_length.  No HIP call. */
long long smfft_pfb_spec_spectra(long long signal_length, int n_channels, int taps_per_channel, int n_integrate);
long long smfft_pfb_real_spec_spectra(long long signal_length, int n_channels, int taps_per_channel, int n_integrate);

/* Integrates n_streams streams, enqueued on hip_stream (a hipStream_t; NULL = the null stream).  Launch only: no synchronisation. */
int smfft_pfb_spec_launch(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                          int n_integrate, void* d_output, void* hip_stream);
int smfft_pfb_real_spec_launch(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                               int n_integrate, void* d_output, void* hip_stream);

/* The same launch on the null stream, timed with events: ADDS the elapsed milliseconds to *FFT_time (when the launch was made and
 * FFT_time is not NULL) and returns after the kernel has finished. */
int smfft_pfb_spec_benchmark(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                             int n_integrate, void* d_output, double* FFT_time);
int smfft_pfb_real_spec_benchmark(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                                  int n_integrate, void* d_output, double* FFT_time);

/* Tuning and tests only: the launch on a grid of at most max_workgroups workgroups (>= 1; 0 = the shipped grid, what *_launch passes:
 * as many workgroups as the device holds at once).  The results do not depend on it, to the bit.  An argument, not a process-wide
 * setting: launches on different streams cannot disturb each other. */
int smfft_pfb_spec_launch_tuned(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                                int n_integrate, void* d_output, void* hip_stream, int max_workgroups);
int smfft_pfb_real_spec_launch_tuned(const void* d_signal, long long signal_length, int n_streams, const void* d_taps, int n_channels, int taps_per_channel,
                                     int n_integrate, void* d_output, void* hip_stream, int max_workgroups);

#ifdef __cplusplus
}
#endif

#endif /* SMFFT_PFB_SPEC_H_ */

/*
 * smfft_fir_detect.h -- C ABI of libsmfft_fir_detect.so: the DETECTED outputs of the overlap-save FIR filter banks for complex signals
 * and complex taps, with segments of N = 256 ... 4096, in one kernel from segment load to detected output.
 *
 * A library of its own, beside libsmfft_amd.so, whose smfft_fir_launch writes the C*K*L complex samples y_{c,k}[n] themselves.  A
 * matched-filter bank (template searches, acceleration or dedispersion trials, pulse compression) wants their power, and very often
 * only the largest power over the filters and the filter that gave it.  These launches compute the y that smfft_fir_launch defines --
 * the same loads, transforms and products, rounded alike in both launches here (against smfft_fir_launch's own output y agrees within
 * that bank's error bound, not necessarily to the last bit) -- and store
 *   power:  p[(c*K + k)*L + n] = |y_{c,k}[n]|^2 = fmaf(re, re, im*im), one float: half the output bytes, and no second pass;
 *   peak:   peak[c*L + n] = max_k p[c,k,n] and index[c*L + n] = the lowest k that attains it: 1/K of the output bytes, no C*K*L
 *           workspace at all.  A NaN power counts as larger than every number, and the first NaN wins: the rule of np.max / np.argmax
 *           along the filter axis, NaN included.  peak's bits are those of the power launch's maximum.
 * 
 *
 * There is no prepare function here: the spectra are those of smfft_fir_prepare (include/smfft.h) in the same mode,
 *   d_spectra: K x N float2, H_k[j] = DFT_N(pad_N(g_k))[j] / N, natural order, g_k = h_k (convolve), g_k[m] = conj(h_k[M-1-m]) (correlate).
 *
 * The other contracts are those of the "FIR filter banks" of include/smfft.h:
 *   - signal d_signal: C channels x L float2, channel c at element c*L (L = signal_length, any value >= 1, 64-bit offsets);
 *   - y as smfft_fir_launch defines it, in both modes (correlate == 0: np.convolve(x_c, h_k)[:L]; correlate != 0:
 *     np.correlate(np.r_[x_c, zeros(M-1)], h_k, 'valid')), 1 <= M = n_taps <= FFT_size - 1;
 *   - d_power: C*K*L float; d_peak: C*L float; d_index: C*L int32 (every index lies in [0, K));
 *   - FFT_size N = 256, 512, 1024, 2048 or 4096;
 *   - buffer contract: signal and spectra 8-byte aligned, the outputs 4-byte aligned (interior pointers are fine); only
 *     signal[0, C*L), spectra[0, K*N) and power[0, C*K*L) -- or peak[0, C*L) and index[0, C*L) -- are touched, and every output element
 *     is written exactly once; inputs and outputs must not overlap.  No workspace and no allocation inside a call, so a launch can be
 *     captured into a graph.
 * Return values: 0, a hipError_t, or -1 -- before any HIP call -- for an unsupported combination (FFT_size not one of the five
 * lengths, n_taps < 1 or >= FFT_size, a count <= 0, signal_length < 0).  signal_length == 0 launches nothing and returns 0.
 *
 * Work split.  The power launch splits its filters into groups by the rule of smfft_fir_launch.  The peak launch cannot: the
 * workgroup that owns a segment must see all K filters, so there is ONE filter group, and a short signal with many filters fills fewer
 * workgroups here than in smfft_fir_launch (C * ceil(L / (N - M + 1)) * N / 4096 of them, whatever K is).
 * Registers.  Every kernel runs at the complex bank's occupancy, two waves per SIMD (at most 256 VGPRs), without scratch and with the
 * complex bank's 34,816 B of LDS: the peak kernel keeps its winners in registers at every length.
 *
 * Out of scope:
 *   - real signals (libsmfft_fir_real.so filters them; its outputs are not detected here);
 *   - N >= 8192 (libsmfft_large_fir.so serves complex data there, undetected);
 *   - thresholded candidate lists (a compaction of the samples above a threshold: the peak outputs are dense, C*L each);
 *   - a maximum over samples rather than filters (per filter, over n): that is a reduction across segments and workgroups.
 */
#ifndef SMFFT_FIR_DETECT_H_
#define SMFFT_FIR_DETECT_H_

#ifdef __cplusplus
extern "C" {
#endif

/* d_power[(c*K + k)*L + n] = |y_{c,k}[n]|^2 of n_channels signals of signal_length samples and the n_filters prepared spectra, enqueued
 * on hip_stream (a hipStream_t; NULL = the null stream).  Launch only: no synchronisation. */
int smfft_fir_power_launch(const void* d_signal, long long signal_length, int n_channels, const void* d_spectra, int n_filters, int n_taps,
                           int FFT_size, int correlate, void* d_power, void* hip_stream);

/* The same launch on the null stream, timed with events: ADDS the elapsed milliseconds to *FFT_time (when the launch was made and
 * FFT_time is not NULL) and returns after the kernel has finished. */
int smfft_fir_power_benchmark(const void* d_signal, long long signal_length, int n_channels, const void* d_spectra, int n_filters, int n_taps,
                              int FFT_size, int correlate, void* d_power, double* FFT_time);

/* d_peak[c*L + n] = max_k |y_{c,k}[n]|^2 and d_index[c*L + n] = the lowest k that attains it, enqueued on hip_stream.  Launch only:
 * no synchronisation. */
int smfft_fir_peak_launch(const void* d_signal, long long signal_length, int n_channels, const void* d_spectra, int n_filters, int n_taps,
                          int FFT_size, int correlate, void* d_peak, void* d_index, void* hip_stream);

/* The same launch on the null stream, timed with events, as smfft_fir_power_benchmark. */
int smfft_fir_peak_benchmark(const void* d_signal, long long signal_length, int n_channels, const void* d_spectra, int n_filters, int n_taps,
                             int FFT_size, int correlate, void* d_peak, void* d_index, double* FFT_time);

#ifdef __cplusplus
}
#endif

#endif /* SMFFT_FIR_DETECT_H_ */

/*
 * smfft_large_fir.h -- C ABI of libsmfft_large_fir.so: overlap-save FIR filter banks with segments of N = 8192 and 16384, for
 * filters of up to 16383 taps, in one kernel from segment load to filtered output.
 *
 * A library of its own, beside libsmfft_amd.so (whose smfft_fir_* stop at N = 4096: at most 4095 taps) and libsmfft_large.so (the
 * bare transforms of these lengths).  A segment is transformed whole in one workgroup's LDS by the engine of libsmfft_large.so,
 * multiplied by a filter's spectrum in registers, transformed back and stored: nothing but the signal, the spectra and the outputs
 * touches memory (include/smfft/smfft_large_fir.hpp).
 *
 * The semantics, layouts, spectra format and return codes are those of the "FIR filter banks" of include/smfft.h:
 *   - signal d_signal: C channels x L float2, channel c at element c*L (L = signal_length, any value >= 1, 64-bit offsets);
 *   - taps d_taps: K x M float2, filter k at element k*M, 1 <= M = n_taps <= FFT_size - 1;
 *   - output d_output: C*K*L float2, y[(c*K + k)*L + n], n < L:
 *       correlate == 0:  y = sum_{m<M} h_k[m] x_c[n - m], x_c[i < 0] = 0         = np.convolve(x_c, h_k)[:L]
 *       correlate != 0:  y = sum_{m<M} conj(h_k[m]) x_c[n + m], x_c[i >= L] = 0  = np.correlate(np.r_[x_c, zeros(M-1)], h_k, 'valid')
 *   - FFT_size N = 8192 or 16384: each channel is cut into S = ceil(L / V) segments of N samples, V = N - M + 1 new outputs each;
 *   - spectra d_spectra: K x N float2, public, so that a caller may produce them any other way:
 *       H_k[j] = DFT_N(pad_N(g_k))[j] / N, natural order, un-normalised forward sign (exp(-2 pi i jm/N)),
 *       g_k = h_k (convolve), g_k[m] = conj(h_k[M-1-m]) (correlate).
 *     The spectra depend on the mode, so prepare and launch must be called with the same `correlate`;
 *   - buffer contract: pointers 8-byte aligned (interior pointers are fine); only signal[0, C*L), taps[0, K*M), spectra[0, K*N) and
 *     out[0, C*K*L) are touched; signal, spectra and output must not overlap.  No workspace and no allocation inside a call, so a
 *     launch can be captured into a graph.
 * Return values: 0, a hipError_t, or -1 -- before any HIP call -- for an unsupported combination (FFT_size not 8192 / 16384,
 * n_taps < 1 or >= FFT_size, a count <= 0, signal_length < 0).  signal_length == 0 launches nothing and returns 0.
 */
#ifndef SMFFT_LARGE_FIR_H_
#define SMFFT_LARGE_FIR_H_

#ifdef __cplusplus
extern "C" {
#endif

/* d_spectra = the prepared form of d_taps, enqueued on hip_stream (a hipStream_t; NULL = the null stream).  Launch only: no
 * synchronisation, no workspace. */
int smfft_large_fir_prepare(const void* d_taps, int n_taps, int n_filters, int FFT_size, int correlate, void* d_spectra, void* hip_stream);

/* Filters n_channels signals of signal_length samples by the n_filters prepared spectra, enqueued on hip_stream.  Launch only: no
 * synchronisation.  Every output element is written exactly once. */
int smfft_large_fir_launch(const void* d_signal, long long signal_length, int n_channels, const void* d_spectra, int n_filters, int n_taps,
                           int FFT_size, int correlate, void* d_output, void* hip_stream);

/* The same launch on the null stream, timed with events: ADDS the elapsed milliseconds to *FFT_time (when the launch was made and
 * FFT_time is not NULL) and returns after the kernel has finished. */
int smfft_large_fir_benchmark(const void* d_signal, long long signal_length, int n_channels, const void* d_spectra, int n_filters, int n_taps,
                              int FFT_size, int correlate, void* d_output, double* FFT_time);

#ifdef __cplusplus
}
#endif

#endif /* SMFFT_LARGE_FIR_H_ */

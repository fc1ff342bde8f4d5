/*
 * smfft_fir_real.h -- C ABI of libsmfft_fir_real.so: overlap-save FIR filter banks for REAL signals and REAL taps, with segments of
 * N = 256 ... 4096, in one kernel from segment load to filtered output.
 *
 * A library of its own, beside libsmfft_amd.so, whose smfft_fir_* take complex64 signals and taps only.  For a real filter g,
 * conv(x1 + i x2, g) = conv(x1, g) + i conv(x2, g): two consecutive real segments of one channel ride in the real and the imaginary
 * lane of one complex N-point transform, so one transform pair filters 2 (N - M + 1) real samples, and the signal and the outputs are
 * float32 -- half the bytes of the complex bank on the cast signal.
 *
 * The semantics and return codes are those of the "FIR filter banks" of include/smfft.h, on real data:
 *   - signal d_signal: C channels x L float, channel c at element c*L (L = signal_length, any value >= 1, 64-bit offsets);
 *   - taps d_taps: K x M float, filter k at element k*M, 1 <= M = n_taps <= FFT_size - 1;
 *   - output d_output: C*K*L float, y[(c*K + k)*L + n], n < L:
 *       correlate == 0:  y = sum_{m<M} h_k[m] x_c[n - m], x_c[i < 0] = 0         = np.convolve(x_c, h_k)[:L]
 *       correlate != 0:  y = sum_{m<M} h_k[m] x_c[n + m], x_c[i >= L] = 0        = np.correlate(np.r_[x_c, zeros(M-1)], h_k, 'valid')
 *   - FFT_size N = 256, 512, 1024, 2048 or 4096: each channel is cut into S = ceil(L / V) segments of N samples, V = N - M + 1 new
 *     outputs each, and consecutive segments 2p, 2p + 1 of a channel into ceil(S / 2) pairs; a pair never spans two channels;
 *   - spectra d_spectra: K x N float2, the format of smfft_fir_prepare:
 *       H_k[j] = DFT_N(pad_N(g_k))[j] / N, natural order, un-normalised forward sign (exp(-2 pi i jm/N)),
 *       g_k = h_k (convolve), g_k[m] = h_k[M-1-m] (correlate).
 *     Spectra from either prepare function (smfft_fir_prepare of the taps cast to complex64, or smfft_fir_real_prepare) may be passed
 *     to either launch (smfft_fir_launch, smfft_fir_real_launch).  The launch reads all N values as given: it neither exploits nor
 *     enforces their Hermitian symmetry.  The spectra depend on the mode, so prepare and launch must be called with the same
 *     `correlate`;
 *   - buffer contract: signal, taps and output 4-byte aligned, spectra 8-byte aligned (interior pointers are fine); only
 *     signal[0, C*L), taps[0, K*M), spectra[0, K*N) and out[0, C*K*L) are touched; signal, spectra and output must not overlap.  No
 *     workspace and no allocation inside a call, so a launch can be captured into a graph.
 * Return values: 0, a hipError_t, or -1 -- before any HIP call -- for an unsupported combination (FFT_size not one of the five
 * lengths, n_taps < 1 or >= FFT_size, a count <= 0, signal_length < 0).  signal_length == 0 launches nothing and returns 0.
 *
 * Out of scope:
 *   - complex taps on real signals: the pairing needs a real g (a complex g mixes the two lanes), so cast the signal and use
 *     smfft_fir_*;
 *   - N >= 8192 (libsmfft_large_fir.so serves complex data there);
 *   - isolation inside a pair: a NaN or Inf sample poisons every output of its PAIR of segments (both segments, every filter, that
 *     channel only), not of its segment alone, and the rounding error of an output scales with the norm of the pair.
 */
#ifndef SMFFT_FIR_REAL_H_
#define SMFFT_FIR_REAL_H_

#ifdef __cplusplus
extern "C" {
#endif

/* d_spectra = the prepared form of d_taps, enqueued on hip_stream (a hipStream_t; NULL = the null stream).  Launch only: no
 * synchronisation, no workspace. */
int smfft_fir_real_prepare(const void* d_taps, int n_taps, int n_filters, int FFT_size, int correlate, void* d_spectra, void* hip_stream);

/* Filters n_channels signals of signal_length samples by the n_filters prepared spectra, enqueued on hip_stream.  Launch only: no
 * synchronisation.  Every output element is written exactly once. */
int smfft_fir_real_launch(const void* d_signal, long long signal_length, int n_channels, const void* d_spectra, int n_filters, int n_taps,
                          int FFT_size, int correlate, void* d_output, void* hip_stream);

/* The same launch on the null stream, timed with events: ADDS the elapsed milliseconds to *FFT_time (when the launch was made and
 * FFT_time is not NULL) and returns after the kernel has finished. */
int smfft_fir_real_benchmark(const void* d_signal, long long signal_length, int n_channels, const void* d_spectra, int n_filters, int n_taps,
                             int FFT_size, int correlate, void* d_output, double* FFT_time);

#ifdef __cplusplus
}
#endif

#endif /* SMFFT_FIR_REAL_H_ */

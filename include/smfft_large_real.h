/*
 * smfft_large_real.h -- C ABI of libsmfft_large_real.so: batched R2C / C2R FFTs of real N = 16384 and 32768 in one pass through HBM.
 *
 * A library of its own, beside libsmfft_amd.so (whose R2C / C2R stop at N = 4096) and libsmfft_large.so (complex 8192 / 16384).
 * Each real FFT of N = 2L points is a complex FFT of L = 8192 / 16384 points, done whole in one workgroup's LDS by the engine of
 * libsmfft_large.so, plus a Hermitian split (R2C) or merge (C2R) through the same LDS image: one read of N * 4 bytes and one write of
 * N * 4 bytes per FFT (include/smfft/smfft_large_real.hpp).
 *
 * Conventions (those of smfft_rc_external_benchmark, so that a caller can switch by length):
 *   - FFT_size is the REAL length N; FFT f of either buffer is at byte f * N * 4 (64-bit offsets);
 *   - inverse = 0 (R2C): N floats x -> N/2 float2 in the packed layout: element 0 = (X[0].re, X[N/2].re), element k = X[k] =
 *     sum x[n] e^{-2 pi i nk/N}, k = 1 .. N/2 - 1;
 *   - inverse != 0 (C2R): the packed layout -> N floats = (N/2) x, x = irfft of the spectrum; X[0] = element 0's real part and
 *     X[N/2] = its imaginary part are taken as real.  C2R(R2C(x)) = (N/2) x;
 *   - natural order in and out;
 *   - buffer contract: pointers 8-byte aligned (interior pointers are fine); only FFTs [0, nFFTs) of either buffer are read or
 *     written; d_output == d_input is allowed, partial overlap is not; the input is left untouched unless it is the output.
 */
#ifndef SMFFT_LARGE_REAL_H_
#define SMFFT_LARGE_REAL_H_

#ifdef __cplusplus
extern "C" {
#endif

/* d_output[f] = R2C (inverse = 0) or C2R (inverse != 0) of d_input[f], f < nFFTs, enqueued on hip_stream (a hipStream_t; NULL =
 * the null stream).  Launch only: no synchronisation.  Returns 0, a hipError_t of the launch, or -1 -- before any HIP call -- for
 * FFT_size not 16384 / 32768 or nFFTs < 0.  nFFTs = 0 launches nothing. */
int smfft_large_real_launch(const void* d_input, void* d_output, int FFT_size, int nFFTs, int inverse, void* hip_stream);

/* The same launch on the null stream, timed with events: ADDS the elapsed milliseconds to *FFT_time (when the launch was made
 * and FFT_time is not NULL) and returns after the kernel has finished.  Same return values. */
int smfft_large_real_benchmark(const void* d_input, void* d_output, int FFT_size, int nFFTs, int inverse, double* FFT_time);

/* The persistent grid a launch of FFT_size uses on the current device when nFFTs is at least as large (workgroups: two per CU at
 * 16384, one at 32768); -1 for an unsupported FFT_size (before any HIP call), 0 when the device cannot be queried. */
int smfft_large_real_grid(int FFT_size);

#ifdef __cplusplus
}
#endif

#endif /* SMFFT_LARGE_REAL_H_ */

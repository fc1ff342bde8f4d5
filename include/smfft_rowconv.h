/*
 * smfft_rowconv.h -- C ABI of libsmfft_rowconv.so: batched linear convolution or correlation of PAIRS of complex rows, a[r] with b[r]
 * for every r, n_a, n_b >= 1 and n_a + n_b - 1 <= 4096, in one kernel and one pass through HBM (two forward transforms, a product and
 * an inverse transform on the register engine's power-of-two transforms).
 *
 * A library of its own, beside the FIR banks, libsmfft_bluestein.so and libsmfft_czt.so, which all multiply the spectrum by something
 * known before the launch (K prepared filter spectra, tables built on the host).  Here the second operand is data too: the
 * cross-correlation of two receivers' blocks, a template per trial, an adaptive filter whose taps change every block, an
 * autocorrelation.  There is no plan, no table and no workspace.
 *
 * Definition.  Rows are float2.  Row r of a is at element r*n_a.  Row r of b is at element r*n_b.  Row r of the output is at element
 * r*m.  All offsets are 64-bit.  Let Lfull = n_a + n_b - 1.
 *   convolve  (correlate == 0):  y[r][k] = sum_j a[r][j] * b[r][k - j]                        for 0 <= k < Lfull.
 *                                This is np.convolve(a[r], b[r]).
 *   correlate (correlate != 0):  y[r][k] = sum_j a[r][j + k - (n_b - 1)] * conj(b[r][j]).
 *                                This is np.correlate(a[r], b[r], 'full'), so lag k - (n_b - 1) sits at index k.  It equals
 *                                np.convolve(a[r], conj(b[r][::-1])).
 *   window:                      the launch stores out[r*m + i] = y[r][first + i] for 0 <= i < m, with 0 <= first, 1 <= m and
 *                                first + m <= Lfull.  A caller who needs +-d lags of a long correlation writes 2d+1 values per row,
 *                                not Lfull.
 * (Terms whose index falls outside a row are zero.)
 *
 * Algorithm.  M = smfft_rowconv_fft_size(n_a, n_b) is the smallest of 256, 512, 1024, 2048, 4096 with M >= Lfull, so the circular
 * convolution of length M of the two zero-padded rows is the linear one.  Per row the kernel loads a, loads the second operand -- b,
 * or in correlate mode conj(b) reversed, so the kernel is always a convolution and the output needs no wrap-around -- scaled by 1 / M
 * (an exact power of two), runs a forward transform of each, multiplies the spectra, runs the inverse transform and stores the
 * elements of the window.  256 threads hold 4096 / M rows per workgroup; workgroups stride over the tiles.  (DESIGN.md section 20,
 * INTEGRATION.md section C13.)
 *
 * Buffer contract: 8-byte alignment; only a[0, batch*n_a), b[0, batch*n_b) and out[0, batch*m) are touched, and every output element
 * is written exactly once.  d_a == d_b is allowed: with correlate set it gives the autocorrelation.  d_out == d_a and d_out == d_b are
 * refused, for an empty batch too, and any other overlap of the output with an input is not allowed.  Rows do not see each other (a
 * NaN stays in its row pair), and a pair with an all-zero row and a finite partner stores +0 in every element.  The launches allocate
 * nothing and do not synchronise, so they can be captured into a graph.
 *
 * Return values: 0, a hipError_t, or -1 -- before any HIP call -- for n_a < 1, n_b < 1 or n_a + n_b - 1 > 4096; first < 0, m < 1 or
 * first + m > Lfull; batch < 0; grid < 1 (launch_tuned); d_out == d_a or d_out == d_b.  batch == 0 launches nothing and returns 0.
 *
 * Out of scope:
 *   - real rows (two real rows in one complex transform need a Hermitian split across threads);
 *   - Lfull > 4096 (that is the large engine's ground);
 *   - one b shared by all rows (that is smfft_fir_*);
 *   - a peak / arg-max output over the lags;
 *   - shrinking M for narrow windows;
 *   - strided rows.
 */
#ifndef SMFFT_ROWCONV_H_
#define SMFFT_ROWCONV_H_

#ifdef __cplusplus
extern "C" {
#endif

/* M, the length of the three transforms inside the kernel: the smallest of 256 ... 4096 with M >= n_a + n_b - 1; -1 for n_a < 1,
 * n_b < 1 or n_a + n_b - 1 > 4096. */
int smfft_rowconv_fft_size(int n_a, int n_b);

/* batch convolutions (correlate == 0) or correlations (correlate != 0) of rows of n_a with rows of n_b elements, elements
 * first ... first + m - 1 of each result, enqueued on hip_stream (a hipStream_t; NULL = the null stream).  Launch only: no allocation,
 * no synchronisation. */
int smfft_rowconv_launch(const void* d_a, const void* d_b, void* d_out, int n_a, int n_b, int first, int m, long long batch, int correlate, void* hip_stream);

/* The same launch with the number of workgroups given (1 <= grid; the default is min(ceil(batch * M / 4096), 12288), grid-strided
 * beyond).  The result does not depend on grid, to the bit. */
int smfft_rowconv_launch_tuned(const void* d_a, const void* d_b, void* d_out, int n_a, int n_b, int first, int m, long long batch, int correlate, void* hip_stream, int grid);

/* The same launch on the null stream, timed with events: ADDS the elapsed milliseconds to *FFT_time (when the launch was made and
 * FFT_time is not NULL) and returns after the kernel has finished. */
int smfft_rowconv_benchmark(const void* d_a, const void* d_b, void* d_out, int n_a, int n_b, int first, int m, long long batch, int correlate, double* FFT_time);

#ifdef __cplusplus
}
#endif

#endif /* SMFFT_ROWCONV_H_ */

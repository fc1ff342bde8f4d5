/*
 * smfft_rowconv_real.h -- C ABI of libsmfft_rowconv_real.so: batched linear convolution or correlation of PAIRS of real rows, a[r] with
 * b[r] for every r, n_a, n_b >= 1 and n_a + n_b - 1 <= 4096, in one kernel and one pass through HBM (one forward transform of the pair,
 * a product and one inverse transform on the register engine's power-of-two transforms).
 *
 * The real-row form of libsmfft_rowconv.so (include/smfft_rowconv.h), in a library of its own: float32 rows in, float32 rows out, half
 * the bytes of the complex library on cast rows and two transforms per pair where it runs three.  Both operands are data: digitiser
 * blocks of two receivers, audio, time series, the operands of np.convolve and np.correlate.  There is no plan, no table and no
 * workspace.
 *
 * Definition.  Rows are float32.  Row r of a is at element r*n_a.  Row r of b is at element r*n_b.  Row r of the output is at element
 * r*m.  All offsets are 64-bit.  Let Lfull = n_a + n_b - 1.
 *   convolve  (correlate == 0):  y[r][k] = sum_j a[r][j] * b[r][k - j]                        for 0 <= k < Lfull.
 *                                This is np.convolve(a[r], b[r]).
 *   correlate (correlate != 0):  y[r][k] = sum_j a[r][j + k - (n_b - 1)] * b[r][j].
 *                                This is np.correlate(a[r], b[r], 'full'), so lag k - (n_b - 1) sits at index k.  It equals
 *                                np.convolve(a[r], b[r][::-1]).
 *   window:                      the launch stores out[r*m + i] = y[r][first + i] for 0 <= i < m, with 0 <= first, 1 <= m and
 *                                first + m <= Lfull.  A caller who needs +-d lags of a long correlation writes 2d+1 values per row,
 *                                not Lfull.
 * (Terms whose index falls outside a row are zero.)
 *
 * Algorithm.  M = smfft_rowconv_real_fft_size(n_a, n_b) is the smallest of 256, 512, 1024, 2048, 4096 with M >= Lfull -- the same
 * function as smfft_rowconv_fft_size.  Per row pair the kernel loads a into the real lane and the second operand -- b, or in correlate
 * mode b reversed -- into the imaginary lane of ONE forward transform, z = a + i b'; recovers the two spectra from Z[k] and Z[M - k];
 * multiplies them; runs one inverse transform, whose real part is the answer; and stores the elements of the window.  One row pair per
 * transform slot: 256 threads hold 4096 / M pairs per workgroup; workgroups stride over the tiles.
 *
 * Balancing.  The two rows of a pair share one fp32 number system inside the transform, so the kernel first scales each by a power of
 * two chosen from that row's own energy (sum of squares in [1, 4) afterwards) and takes the two exponents off the result with one
 * ldexp.  Without it a row whose energy is 2^24 below its partner's would lose five digits.  The scales are exact powers of two:
 * scaling a[r] or b[r] by 2^s scales row r of the result by 2^s to the bit, as long as nothing leaves the normal fp32 range.
 * 
 *
 * Buffer contract: 4-byte alignment; only a[0, batch*n_a), b[0, batch*n_b) and out[0, batch*m) are touched, and every output element
 * is written exactly once.  d_a == d_b is allowed: with correlate set it gives the autocorrelation.  d_out == d_a and d_out == d_b are
 * refused, for an empty batch too, and any other overlap of the output with an input is not allowed.  The launches allocate nothing
 * and do not synchronise, so they can be captured into a graph.
 *
 * Row contract: the bits of row r's outputs depend only on a[r], b[r], n_a, n_b and the mode -- not on the batch, the row's position
 * in it, the grid or the window; a window is the slice of the full result, to the bit.  A NaN or Inf anywhere in a pair makes all
 * outputs of that pair NaN and touches no other row.  A pair with an all-zero row and a finite partner stores +0 in every element.
 *
 * Return values: 0, a hipError_t, or -1 -- before any HIP call -- for n_a < 1, n_b < 1 or n_a + n_b - 1 > 4096; first < 0, m < 1 or
 * first + m > Lfull; batch < 0; grid < 1 (launch_tuned); d_out == d_a or d_out == d_b.  batch == 0 launches nothing and returns 0.
 *
 * Out of scope:
 *   - complex rows (that is smfft_rowconv_*);
 *   - two row pairs in one transform slot (it would halve the transforms again and break the row contract);
 *   - results or intermediate sums outside the normal fp32 range (a result that is subnormal is rounded once, by the final ldexp);
 *   - Lfull > 4096 (that is the large engine's ground);
 *   - one b shared by all rows (that is smfft_fir_real_*);
 *   - a peak / arg-max output over the lags;
 *   - shrinking M for narrow windows;
 *   - strided rows.
 */
#ifndef SMFFT_ROWCONV_REAL_H_
#define SMFFT_ROWCONV_REAL_H_

#ifdef __cplusplus
extern "C" {
#endif

/* M, the length of the two transforms inside the kernel: the smallest of 256 ... 4096 with M >= n_a + n_b - 1; -1 for n_a < 1,
 * n_b < 1 or n_a + n_b - 1 > 4096. */
int smfft_rowconv_real_fft_size(int n_a, int n_b);

/* batch convolutions (correlate == 0) or correlations (correlate != 0) of float32 rows of n_a with rows of n_b elements, elements
 * first ... first + m - 1 of each result, enqueued on hip_stream (a hipStream_t; NULL = the null stream).  Launch only: no allocation,
 * no synchronisation. */
int smfft_rowconv_real_launch(const void* d_a, const void* d_b, void* d_out, int n_a, int n_b, int first, int m, long long batch, int correlate, void* hip_stream);

/* The same launch with the number of workgroups given (1 <= grid; the default is min(ceil(batch * M / 4096), 12288), grid-strided
 * beyond).  The result does not depend on grid, to the bit. */
int smfft_rowconv_real_launch_tuned(const void* d_a, const void* d_b, void* d_out, int n_a, int n_b, int first, int m, long long batch, int correlate, void* hip_stream, int grid);

/* The same launch on the null stream, timed with events: ADDS the elapsed milliseconds to *FFT_time (when the launch was made and
 * FFT_time is not NULL) and returns after the kernel has finished. */
int smfft_rowconv_real_benchmark(const void* d_a, const void* d_b, void* d_out, int n_a, int n_b, int first, int m, long long batch, int correlate, double* FFT_time);

#ifdef __cplusplus
}
#endif

#endif /* SMFFT_ROWCONV_REAL_H_ */

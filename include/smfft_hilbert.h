/*
 * smfft_hilbert.h -- C ABI of libsmfft_hilbert.so: batched Hilbert transform, analytic signal and envelope of real rows of
 * n = 512, 1024, 2048, 4096 or 8192 points, in one kernel and one pass through HBM (n floats in and n floats -- the analytic signal:
 * n complex64 -- out per row, two complex transforms of M = n / 2 points of the register engine per row).
 *
 * Definition.  Rows are float32 and contiguous: row r is at element r*n of d_in and of d_out.  All offsets are 64-bit.
 * With X = DFT_n(x):
 *   H(x) = IDFT_n(-i s[k] X[k]), s[k] = +1 for 0 < k < n/2, -1 for n/2 < k < n, 0 at k = 0 and k = n/2,
 * which is exactly scipy.signal.hilbert(x).imag.  The kind selects the output:
 *   SMFFT_HILBERT_QUADRATURE (0):  H(x), n floats per row
 *   SMFFT_HILBERT_ANALYTIC   (1):  a = x + i H(x), n interleaved complex64 per row (re, im, re, im ...).  The real part is the input
 *                                  to the bit; scipy's is only close to it (scipy takes it through both transforms)
 *   SMFFT_HILBERT_ENVELOPE   (2):  sqrt(x^2 + H(x)^2), n floats per row
 *
 * Algorithm.  Consecutive pairs of samples are the two lanes of a complex transform of M = n / 2 points, z[p] = x[2p] + i x[2p+1];
 * Z = DFT_M(z); with the partner P[k] = conj Z[(M-k) mod M] and W_n = exp(-2 pi i / n),
 *   Z'[k] = (conj(W_n^k) (Z[k] + P[k]) - W_n^k (Z[k] - P[k])) / n, Z'[0] = 0
 * merges the Hermitian split, the multiplier -i s[k], the zeroed bins 0 and n/2 and the merge of a C2R transform; the un-normalised
 * inverse transform z' of Z' holds H(x)[2p] = Re z'[p] and H(x)[2p+1] = Im z'[p].  All twiddles are fp64 values rounded once to fp32;
 * 1/n is a power of two and exact.  One row per transform slot: 256 threads hold 8192 / n rows per workgroup; workgroups stride over
 * the tiles.  There is no plan, no table to prepare and no workspace.  
 *
 * Buffer contract: 4-byte alignment of d_in and of a float output, 8-byte alignment of the complex64 output; only in[0, batch*n) and
 * the output's batch*n elements are touched, and every output element is written exactly once.  In place, d_out == d_in, is allowed
 * for kinds 0 and 2: a workgroup holds its rows in registers before it stores any of them, and a row belongs to one workgroup.
 * Ranges that overlap without being equal are refused, and so is any overlap for kind 1, whose output is twice the input.  The
 * launches allocate nothing and do not synchronise, so they can be captured into a graph.
 *
 * Row contract: the bits of row r's outputs depend only on x[r], n and kind -- not on the batch, the row's position in it, the grid,
 * or whether the launch is in place.  A NaN or Inf in a row stays in that row.
 *
 * Return values: 0, a hipError_t, or -1 -- before any HIP call -- for n not one of the five lengths; kind outside 0 ... 2;
 * batch < 0; grid < 1 (launch_tuned); d_in overlapping the output's batch*n*4 bytes (kind 1: batch*n*8) other than in place with
 * kinds 0 and 2.  batch == 0 launches nothing and returns 0.
 *
 * Out of scope:
 *   - n < 512, n > 8192 and n that is not a power of two;
 *   - complex input;
 *   - a user-supplied frequency response;
 *   - instantaneous phase or frequency;
 *   - orthonormal scaling;
 *   - two-dimensional transforms;
 *   - strided rows, and any element type but float32.
 */
#ifndef SMFFT_HILBERT_H_
#define SMFFT_HILBERT_H_

#ifdef __cplusplus
extern "C" {
#endif

#define SMFFT_HILBERT_QUADRATURE 0
#define SMFFT_HILBERT_ANALYTIC 1
#define SMFFT_HILBERT_ENVELOPE 2

/* M = n / 2, the length of the complex transforms inside the kernel, for n = 512 ... 8192 a power of two; -1 for every other n. */
int smfft_hilbert_fft_size(int n);

/* batch rows of n float32 points from d_in, the output of `kind` to d_out, enqueued on hip_stream (a hipStream_t; NULL = the null
 * stream).  Launch only: no allocation, no synchronisation. */
int smfft_hilbert_launch(const void* d_in, void* d_out, int n, long long batch, int kind, void* hip_stream);

/* The same launch with the number of workgroups given (1 <= grid; the default is min(ceil(batch * n / 8192), 12288), grid-strided
 * beyond).  The result does not depend on grid, to the bit. */
int smfft_hilbert_launch_tuned(const void* d_in, void* d_out, int n, long long batch, int kind, void* hip_stream, int grid);

/* The same launch on the null stream, timed with events: ADDS the elapsed milliseconds to *FFT_time (when the launch was made and
 * FFT_time is not NULL) and returns after the kernel has finished. */
int smfft_hilbert_benchmark(const void* d_in, void* d_out, int n, long long batch, int kind, double* FFT_time);

#ifdef __cplusplus
}
#endif

#endif /* SMFFT_HILBERT_H_ */

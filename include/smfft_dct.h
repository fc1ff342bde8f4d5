/*
 * smfft_dct.h -- C ABI of libsmfft_dct.so: batched discrete cosine and sine transforms of types II and III of real rows of
 * n = 512, 1024, 2048, 4096 or 8192 points, in one kernel and one pass through HBM (n floats in, n floats out per row, one complex
 * transform of M = n / 2 points of the register engine per row).
 *
 * Definition.  Un-normalised, the convention of scipy.fft with norm=None.  Rows are float32 and contiguous: row r is at element r*n
 * of d_in and of d_out.  All offsets are 64-bit.
 *   DCT-II  (type 2, sine == 0):  X[k] = 2 sum_j x[j] cos(pi k (2j+1) / (2n))
 *   DCT-III (type 3, sine == 0):  y[j] = X[0] + 2 sum_{k>=1} X[k] cos(pi k (2j+1) / (2n))
 *   DST-II  (type 2, sine != 0):  X[k] = 2 sum_j x[j] sin(pi (k+1)(2j+1) / (2n))
 *   DST-III (type 3, sine != 0):  y[j] = (-1)^j X[n-1] + 2 sum_{k<n-1} X[k] sin(pi (k+1)(2j+1) / (2n))
 * Type III undoes type II up to a factor: DCT-III(DCT-II(x)) = 2n x and DST-III(DST-II(x)) = 2n x.
 *
 * Algorithm.  The even samples of the row, and the odd samples reversed, are the two lanes of ONE complex transform of M = n / 2
 * points; type II follows it with a Hermitian split and a quarter-wave twiddle in front of the store, type III runs the inverses of
 * those behind the load and an inverse transform.  The sine transforms are the cosine kernels with a sign on the odd samples and the
 * spectrum's index reversed.  All twiddles are fp64 values rounded once to fp32.  One row per transform slot: 256 threads hold
 * 8192 / n rows per workgroup; workgroups stride over the tiles.  There is no plan, no table to prepare and no workspace.
 * 
 *
 * Buffer contract: 4-byte alignment; only in[0, batch*n) and out[0, batch*n) are touched, and every output element is written exactly
 * once.  In place, d_out == d_in, is allowed: a workgroup holds its rows in registers before it stores any of them, and a row belongs
 * to one workgroup.  Ranges that overlap without being equal are refused.  The launches allocate nothing and do not synchronise, so
 * they can be captured into a graph.
 *
 * Row contract: the bits of row r's outputs depend only on x[r], n, type and sine -- not on the batch, the row's position in it, the
 * grid, or whether the launch is in place.  A NaN or Inf in a row stays in that row.
 *
 * Return values: 0, a hipError_t, or -1 -- before any HIP call -- for n not one of the five lengths; type not 2 or 3; batch < 0;
 * grid < 1 (launch_tuned); d_in and d_out overlapping without being equal.  batch == 0 launches nothing and returns 0.
 *
 * Out of scope:
 *   - n < 512, n > 8192 and n that is not a power of two;
 *   - types I and IV;
 *   - orthonormal scaling (norm="ortho": scale X[0] and the rest on the caller's side);
 *   - two-dimensional transforms;
 *   - strided rows, and any element type but float32.
 */
#ifndef SMFFT_DCT_H_
#define SMFFT_DCT_H_

#ifdef __cplusplus
extern "C" {
#endif

/* M = n / 2, the length of the complex transform inside the kernel, for n = 512 ... 8192 a power of two; -1 for every other n. */
int smfft_dct_fft_size(int n);

/* batch transforms of float32 rows of n points: type 2 or 3, the cosine (sine == 0) or the sine (sine != 0) transform, enqueued on
 * hip_stream (a hipStream_t; NULL = the null stream).  Launch only: no allocation, no synchronisation. */
int smfft_dct_launch(const void* d_in, void* d_out, int n, long long batch, int type, int sine, void* hip_stream);

/* The same launch with the number of workgroups given (1 <= grid; the default is min(ceil(batch * n / 8192), 12288), grid-strided
 * beyond).  The result does not depend on grid, to the bit. */
int smfft_dct_launch_tuned(const void* d_in, void* d_out, int n, long long batch, int type, int sine, void* hip_stream, int grid);

/* The same launch on the null stream, timed with events: ADDS the elapsed milliseconds to *FFT_time (when the launch was made and
 * FFT_time is not NULL) and returns after the kernel has finished. */
int smfft_dct_benchmark(const void* d_in, void* d_out, int n, long long batch, int type, int sine, double* FFT_time);

#ifdef __cplusplus
}
#endif

#endif /* SMFFT_DCT_H_ */

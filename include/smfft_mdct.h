/*
 * smfft_mdct.h -- C ABI of libsmfft_mdct.so: batched discrete cosine and sine transforms of type IV of real rows of
 * n = 512, 1024, 2048, 4096 or 8192 points, and the modified discrete cosine transform (MDCT) and its inverse (IMDCT) of
 * N = 512 ... 8192 coefficients per frame of 2N samples, each in one kernel and one pass through HBM (one complex transform of
 * M = n / 2 points of the register engine per row or frame).
 *
 * Definition.  Un-normalised; the type IV transforms follow the convention of scipy.fft with norm=None.  Rows are float32.  All
 * offsets are 64-bit.
 *   DCT-IV (sine == 0):  X[k] = 2 sum_j x[j] cos(pi (2k+1)(2j+1) / (4n))
 *   DST-IV (sine != 0):  X[k] = 2 sum_j x[j] sin(pi (2k+1)(2j+1) / (4n))   = (-1)^k DCT-IV(reverse x)[k]
 *   MDCT:   X[k] = sum_{j<2N} w[j] x[j] cos(pi/N (j + 1/2 + N/2)(k + 1/2)),  k < N
 *   IMDCT:  y[j] = w[j] sum_{k<N} X[k] cos(pi/N (j + 1/2 + N/2)(k + 1/2)),  j < 2N
 * Each type IV transform is its own inverse up to a factor: DCT-IV(DCT-IV(x)) = 2n x.  With a window that satisfies
 * w[j]^2 + w[j+N]^2 = 1, overlap-adding the IMDCT of MDCT frames taken at hop N gives (N/2) x.  The window is a caller-supplied
 * table of 2N floats on the device; NULL means all ones.
 *
 * Algorithm.  t[p] = (x[2p] + i x[n-1-2p]) exp(-i pi (4p+1) / (4n)), p < M = n / 2; T = DFT_M(t); Y[k] = T[k] exp(-i pi k / n);
 * X[2k] = 2 Re Y[k], X[n-1-2k] = -2 Im Y[k]: one twiddle in front of the transform and one behind it, no Hermitian split, the same
 * index map on both sides.  The sine transform reads the row reversed and puts the sign on the store.  The MDCT is half the DCT-IV of
 * the fold u = [-c_r - d, a - b_r] of the windowed frame [a, b, c, d] (quarters of N / 2 samples, _r reversed), formed in front of
 * the first twiddle; the IMDCT is w [D[N/2:], -reverse(D), -D[:N/2]] with D half the DCT-IV of the coefficients, formed behind the
 * second one.  All twiddles are fp64 values rounded once to fp32.  One row or frame per transform slot: 256 threads hold 8192 / n
 * of them per workgroup; workgroups stride over the tiles.  There is no plan, no table to prepare and no workspace.
 * 
 *
 * Buffer contract: 4-byte alignment for every pointer; every output element is written exactly once and nothing else is.
 *   dct4:  row r is at element r*n of d_in and of d_out; only in[0, batch*n) and out[0, batch*n) are touched.  In place,
 *          d_out == d_in, is allowed: a workgroup holds its rows in registers before it stores any of them, and a row belongs to one
 *          workgroup.  Ranges that overlap without being equal are refused.
 *   mdct:  frame (c, f), c < streams, f < frames, reads in[c*stream_stride + f*hop ... + 2N) and writes out[(c*frames + f)*N ... + N).
 *          Frames may overlap each other: hop = N is the lapped transform, and plain rows are frames = 1, stream_stride = 2N.  The
 *          output may overlap neither the input range in[0, (streams-1)*stream_stride + (frames-1)*hop + 2N) nor the window.
 *   imdct: row r reads in[r*N ... + N) and writes out[r*2N ... + 2N), both contiguous; the output may overlap neither the input nor
 *          the window.  There is no overlap-add in the kernel.
 * The launches allocate nothing and do not synchronise, so they can be captured into a graph.
 *
 * Row contract: the bits of a row's or frame's outputs depend only on that row or frame (and the window), n and the transform -- not on
 * the batch, the row's position in it, the grid, or whether the launch is in place.  A NaN or Inf in a row or frame stays in it.
 *
 * Return values: 0, a hipError_t, or -1 -- before any HIP call -- for n or N not one of the five lengths; a negative count (batch,
 * streams, frames); hop < 1 or stream_stride < 1; grid < 1 (launch_tuned); a forbidden overlap.  A zero count launches nothing and
 * returns 0.
 *
 * Out of scope:
 *   - n < 512, n > 8192 and n that is not a power of two;
 *   - type I (types II and III: smfft_dct.h);
 *   - orthonormal scaling;
 *   - overlap-add inside the IMDCT kernel;
 *   - windows other than caller-supplied tables;
 *   - any element type but float32.
 */
#ifndef SMFFT_MDCT_H_
#define SMFFT_MDCT_H_

#ifdef __cplusplus
extern "C" {
#endif

/* M = n / 2, the length of the complex transform inside the kernels, for n = 512 ... 8192 a power of two; -1 for every other n. */
int smfft_mdct_fft_size(int n);

/* batch DCT-IV (sine == 0) or DST-IV (sine != 0) transforms of float32 rows of n points, enqueued on hip_stream (a hipStream_t;
 * NULL = the null stream).  Launch only: no allocation, no synchronisation. */
int smfft_dct4_launch(const void* d_in, void* d_out, int n, long long batch, int sine, void* hip_stream);

/* The same launch with the number of workgroups given (1 <= grid; the default is min(ceil(batch * n / 8192), 12288), grid-strided
 * beyond).  The result does not depend on grid, to the bit. */
int smfft_dct4_launch_tuned(const void* d_in, void* d_out, int n, long long batch, int sine, void* hip_stream, int grid);

/* The same launch on the null stream, timed with events: ADDS the elapsed milliseconds to *FFT_time (when the launch was made and
 * FFT_time is not NULL) and returns after the kernel has finished. */
int smfft_dct4_benchmark(const void* d_in, void* d_out, int n, long long batch, int sine, double* FFT_time);

/* streams * frames MDCTs of N coefficients from frames of 2N float32 samples under the window d_window (2N floats, or NULL). */
int smfft_mdct_launch(const void* d_in, void* d_out, const void* d_window, int N, long long streams, long long frames, long long hop, long long stream_stride, void* hip_stream);
int smfft_mdct_launch_tuned(const void* d_in, void* d_out, const void* d_window, int N, long long streams, long long frames, long long hop, long long stream_stride, void* hip_stream, int grid);
int smfft_mdct_benchmark(const void* d_in, void* d_out, const void* d_window, int N, long long streams, long long frames, long long hop, long long stream_stride, double* FFT_time);

/* batch IMDCTs: rows of N float32 coefficients in, rows of 2N windowed samples out (d_window: 2N floats, or NULL). */
int smfft_imdct_launch(const void* d_in, void* d_out, const void* d_window, int N, long long batch, void* hip_stream);
int smfft_imdct_launch_tuned(const void* d_in, void* d_out, const void* d_window, int N, long long batch, void* hip_stream, int grid);
int smfft_imdct_benchmark(const void* d_in, void* d_out, const void* d_window, int N, long long batch, double* FFT_time);

#ifdef __cplusplus
}
#endif

#endif /* SMFFT_MDCT_H_ */

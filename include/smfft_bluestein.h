/*
 * smfft_bluestein.h -- C ABI of libsmfft_bluestein.so: batched complex-to-complex FFTs of ANY length 1 <= n <= 2048, in one kernel
 * and one pass through HBM (Bluestein's algorithm on the register engine's power-of-two transforms).
 *
 * A library of its own, beside libsmfft_amd.so, whose smfft_launch serves the powers of two 32 ... 4096.  Rows of 1000, 1536 or 2039
 * samples are served here.  Powers of two are accepted as well, but smfft_launch computes them more cheaply (one transform of n
 * points instead of two of M >= 2n - 1): use it for them.
 *
 * Definition.  batch rows of n float2, row r at element r*n (64-bit offsets):
 *   forward:  out[r*n + k] = sum_j in[r*n + j] * exp(-2 pi i j k / n)
 *   inverse:  the same with +, UN-normalised (the library's inverse everywhere: divide by n yourself).
 *
 * Algorithm.  With w[j] = exp(-i pi j^2 / n) and b[j] = conj(w[|j|]),  X[k] = w[k] * sum_j (x[j] w[j]) * b[k - j]: a circular
 * convolution of length M = smfft_bluestein_fft_size(n), the smallest of 256, 512, 1024, 2048, 4096 with M >= 2n - 1 (every n <= 128
 * uses 256, n = 2048 uses 4096).  The kernel is the FIR filter bank's chain with one fixed "filter": load, multiply by w, forward
 * transform of M points, product with the prepared spectrum of b, inverse transform, multiply by w, store the first n elements.  No
 * workspace, no second launch.  
 *
 * The plan: 2M float2 that depend on (n, direction) only, built ONCE per length by smfft_bluestein_prepare (on the device) or
 * smfft_bluestein_tables (in host memory):
 *   W[0, M):  W[j] = exp(-+ i pi (j^2 mod 2n) / n) for j < n (- forward, + inverse), zero beyond;
 *   B[0, M):  DFT_M(b) / M in natural order, b[j] = conj(W[j]) for j < n, b[M - j] = b[j] for 1 <= j < n, zero elsewhere.
 * Both are computed on the host in fp64 (j^2 mod 2n in integers) and rounded once to fp32.  The direction lives in the tables only:
 * the launch takes no direction, and a plan prepared with inverse != 0 makes the same kernel compute the inverse.
 *
 * Buffer contract: 8-byte alignment; only in[0, batch*n), out[0, batch*n) and the plan's 2M float2 are touched, and every output
 * element is written exactly once.  d_out == d_in (in place) is allowed: a workgroup has loaded its rows before it stores them, and
 * rows are disjoint.  Any other overlap of input and output is not allowed.  Rows do not see each other (a NaN stays in its row), and
 * a row of zeros transforms to +0 in every element.  The launches allocate nothing and do not synchronise, so
 * they can be captured into a graph; smfft_bluestein_prepare copies from host memory and waits, so it cannot.
 *
 * Return values: 0, a hipError_t, or -1 -- before any HIP call -- for n < 1, n > 2048, batch < 0 (and grid < 1 for launch_tuned).
 * batch == 0 launches nothing and returns 0.
 *
 * Out of scope:
 *   - n > 2048 (M = 8192 / 16384 is the large engine's ground);
 *   - real input;
 *   - strided or transposed rows;
 *   - a general chirp-z (zoom) transform with arbitrary start and step: other tables, the same kernel;
 *   - routing non-power-of-two lengths through smfft_launch itself.
 */
#ifndef SMFFT_BLUESTEIN_H_
#define SMFFT_BLUESTEIN_H_

#ifdef __cplusplus
extern "C" {
#endif

/* M, the length of the two transforms inside the kernel: the smallest of 256 ... 4096 with M >= 2n - 1; -1 for n outside 1 ... 2048. */
int smfft_bluestein_fft_size(int n);

/* Bytes of the plan of length n: 16 * M (2M float2); -1 for n outside 1 ... 2048. */
long long smfft_bluestein_plan_bytes(int n);

/* Host only, no HIP call: writes the plan of (n, inverse != 0) into the smfft_bluestein_plan_bytes(n) bytes at h_plan (host memory). */
int smfft_bluestein_tables(int n, int inverse, void* h_plan);

/* Builds the plan on the host, copies it to the smfft_bluestein_plan_bytes(n) bytes at d_plan (device memory) on hip_stream (a
 * hipStream_t; NULL = the null stream) and returns once the copy is complete. */
int smfft_bluestein_prepare(int n, int inverse, void* d_plan, void* hip_stream);

/* batch transforms of n points with the prepared plan, enqueued on hip_stream.  Launch only: no allocation, no synchronisation. */
int smfft_bluestein_launch(const void* d_in, void* d_out, int n, long long batch, const void* d_plan, void* hip_stream);

/* The same launch with the number of workgroups given (1 <= grid; the default is min(ceil(batch * M / 4096), 12288), grid-strided
 * beyond).  The result does not depend on grid, to the bit. */
int smfft_bluestein_launch_tuned(const void* d_in, void* d_out, int n, long long batch, const void* d_plan, void* hip_stream, int grid);

/* The same launch on the null stream, timed with events: ADDS the elapsed milliseconds to *FFT_time (when the launch was made and
 * FFT_time is not NULL) and returns after the kernel has finished. */
int smfft_bluestein_benchmark(const void* d_in, void* d_out, int n, long long batch, const void* d_plan, double* FFT_time);

#ifdef __cplusplus
}
#endif

#endif /* SMFFT_BLUESTEIN_H_ */

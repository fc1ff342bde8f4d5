/*
 * smfft_czt.h -- C ABI of libsmfft_czt.so: batched chirp-z (zoom) transforms.  m spectral points on an arbitrary arc of the unit
 * circle from rows of n complex samples, 1 <= n, m <= 2048, in one kernel and one pass through HBM (Bluestein's algorithm on the
 * register engine's power-of-two transforms).
 *
 * A library of its own, beside libsmfft_bluestein.so, whose kernel is specialised to the DFT (m = n, start = 0, step = 1/n: one chirp
 * table, half of a thread's elements).  This one serves fine frequency resolution around a candidate line: m points spaced `step`
 * from `start` on, whatever n is.  It computes the DFT too (start = 0, step = 1/n, m = n), at a price: use
 * smfft_bluestein_launch, or smfft_launch at a power of two, for that.
 *
 * Definition.  batch rows of n float2 in, row r at element r*n; batch rows of m float2 out, row r at element r*m (64-bit offsets):
 *   out[r*m + k] = sum_{j<n} in[r*n + j] * exp(-2 pi i * j * (start + k*step)),   0 <= k < m.
 * start and step are doubles in cycles per sample, any finite value of either sign.  UN-normalised, like every transform of the
 * library.  start = 0, step = 1/n, m = n is the forward DFT; step = -1/n the library's inverse.  There is no direction flag: the
 * direction lives in the tables.
 *
 * Algorithm.  With j k = (j^2 + k^2 - (k - j)^2) / 2:  X[k] = C[k] * sum_j (x[j] A[j]) * b[k - j], a circular convolution of length
 * M = smfft_czt_fft_size(n, m), the smallest of 256, 512, 1024, 2048, 4096 with M >= n + m - 1.  Either of n, m may exceed M / 2.  The
 * kernel: load, multiply by A, forward transform of M points, product with the prepared spectrum of b, inverse transform, multiply by
 * C, store the first m elements.  No workspace, no second launch.  
 *
 * The plan: 3M float2 that depend on (n, m, start, step) only, built ONCE per arc by smfft_czt_prepare (on the device) or
 * smfft_czt_tables (in host memory):
 *   A[0, M):  A[j] = exp(-2 pi i (j start + step j^2 / 2)) for j < n, zero beyond: the input chirp;
 *   B[0, M):  DFT_M(b) / M in natural order, b[t mod M] = exp(+2 pi i step t^2 / 2) for -(n - 1) <= t <= m - 1, zero elsewhere;
 *   C[0, M):  C[k] = exp(-2 pi i step k^2 / 2) for k < m, zero beyond: the output chirp.
 * All three are computed on the host in fp64 and rounded once to fp32.  start is first reduced to [-1/2, 1/2] and step to [-1, 1]
 * (exactly; neither changes a table entry), every phase is formed in cycles and reduced modulo 1 before its cosine and sine are taken.
 *
 * Buffer contract: 8-byte alignment; only in[0, batch*n), out[0, batch*m) and the plan's 3M float2 are touched, and every output
 * element is written exactly once.  d_out == d_in (in place) is allowed only when m == n: a workgroup has loaded its rows before it
 * stores them, and rows of the same length are disjoint; with m != n row r of the output overlaps other rows of the input, and the
 * call is refused.  Any other overlap of input and output is not allowed.  Rows do not see each other (a NaN stays in its row), and a
 * row of zeros transforms to +0 in every element.  The launches allocate nothing and do not synchronise, so they can be captured into
 * a graph; smfft_czt_prepare copies from host memory and waits, so it cannot.
 *
 * Return values: 0, a hipError_t, or -1 -- before any HIP call -- for n or m outside 1 ... 2048, batch < 0, grid < 1 (launch_tuned),
 * a start or step that is not finite (tables, prepare), a null h_plan (tables), and d_out == d_in with m != n.  batch == 0 launches
 * nothing and returns 0.
 *
 * Out of scope:
 *   - spirals off the unit circle, |a| != 1 or |w| != 1 (the tables would grow like |w|^(k^2 / 2): another scaling problem);
 *   - n > 2048 or m > 2048 (M = 8192 / 16384 is the large engine's ground);
 *   - real input;
 *   - strided or transposed rows.
 */
#ifndef SMFFT_CZT_H_
#define SMFFT_CZT_H_

#ifdef __cplusplus
extern "C" {
#endif

/* M, the length of the two transforms inside the kernel: the smallest of 256 ... 4096 with M >= n + m - 1; -1 for n or m outside
 * 1 ... 2048. */
int smfft_czt_fft_size(int n, int m);

/* Bytes of the plan of (n, m): 24 * M (3M float2); -1 for n or m outside 1 ... 2048. */
long long smfft_czt_plan_bytes(int n, int m);

/* Host only, no HIP call: writes the plan of (n, m, start, step) into the smfft_czt_plan_bytes(n, m) bytes at h_plan (host memory). */
int smfft_czt_tables(int n, int m, double start, double step, void* h_plan);

/* Builds the plan on the host, copies it to the smfft_czt_plan_bytes(n, m) bytes at d_plan (device memory) on hip_stream (a
 * hipStream_t; NULL = the null stream) and returns once the copy is complete. */
int smfft_czt_prepare(int n, int m, double start, double step, void* d_plan, void* hip_stream);

/* batch transforms of n samples to m points with the prepared plan, enqueued on hip_stream.  Launch only: no allocation, no
 * synchronisation. */
int smfft_czt_launch(const void* d_in, void* d_out, int n, int m, long long batch, const void* d_plan, void* hip_stream);

/* The same launch with the number of workgroups given (1 <= grid; the default is min(ceil(batch * M / 4096), 12288), grid-strided
 * beyond).  The result does not depend on grid, to the bit. */
int smfft_czt_launch_tuned(const void* d_in, void* d_out, int n, int m, long long batch, const void* d_plan, void* hip_stream, int grid);

/* The same launch on the null stream, timed with events: ADDS the elapsed milliseconds to *FFT_time (when the launch was made and
 * FFT_time is not NULL) and returns after the kernel has finished. */
int smfft_czt_benchmark(const void* d_in, void* d_out, int n, int m, long long batch, const void* d_plan, double* FFT_time);

#ifdef __cplusplus
}
#endif

#endif /* SMFFT_CZT_H_ */

/*
 * smfft_welch.h -- C ABI of libsmfft_welch.so: Welch power spectra and cross spectra of real signals.  The frames of the short-time
 * Fourier transform of smfft_stft.h (n = 512, 1024, 2048, 4096 or 8192 samples at any hop) are summed over T consecutive frames inside
 * the kernel, as |X|^2 of one signal or as conj(X) Y of two, in one kernel and one pass through HBM: the frames' spectra never reach
 * memory, and a launch stores M + 1 values per T frames.
 *
 * Definition.  Samples and window are float32.  All offsets are 64-bit.  With M = n / 2, frame (c, f) reads
 * in[c*stream_stride + f*hop ... + n) under window[0, n) (NULL means all ones), X[c, f, k], k <= M, is the value that
 * smfft_stft_launch(kind = 0) stores for that frame and p[c, f, k] the value that smfft_stft_launch(kind = 1) stores, to the bit.
 *   Auto spectra:   S[(c*groups + g)*(M + 1) + k] = sum_{t<T} p[c, g*T + t, k]                                   float32
 *   Cross spectra:  C[(c*groups + g)*(M + 1) + k] = sum_{t<T} conj(X[c, g*T + t, k]) Y[c, g*T + t, k]            complex64
 *                   (scipy.signal.csd's convention), stream c of x with stream c of y; per term re = xr*yr + xi*yi in one
 *                   expression, im = a - b with a = xr*yi and b = xi*yr rounded on their own.
 * The sums run sequentially in fp32 in frame order, per component: acc = p_0, then acc += p_t, every term rounded to fp32 before the
 * add.  With T = 1 the auto spectra equal smfft_stft_launch(kind = 1) bit for bit.  The real part of csd(x, x) equals the auto
 * spectrum to the bit and its imaginary part is exactly +0.  The imaginary parts of bins 0 and M are stored as exactly +0 in every
 * case: X and Y are real there.
 *
 * Algorithm.  The frame-to-spectrum step of smfft_stft.h (windowed pairs in the two lanes of ONE complex transform of M points of the
 * register engine, partner through LDS, Hermitian split).  A transform slot's unit of work is one (stream, group), not one frame: it
 * loops over the T frames of its group and keeps the running sums of its 16 bins (and of bin M) in registers; the cross kernel
 * transforms x's frame, keeps X in registers, transforms y's frame through the same LDS region and accumulates.  256 threads hold
 * 8192 / n slots per workgroup; workgroups stride over the tiles.  No plan, no table to prepare, no workspace, no atomics and no
 * allocation in a call.  
 *
 * Buffer contract: 4-byte alignment for the signals, the window and the float output, 8-byte alignment for the complex output; every
 * output element is written exactly once and nothing else is.  Group (c, g), c < streams, g < groups, reads frames g*T ... g*T + T - 1
 * of stream c; frames f >= groups*T are never read.  The extent of a signal is
 * in[0, (streams-1)*stream_stride + (groups*T-1)*hop + n).  x_stride >= 1 as in smfft_stft.h; y_stride = 0 is allowed and means one
 * reference stream for all c (its extent is then that of one stream).  d_x and d_y may point into the same buffer, and d_x == d_y is
 * legal.  The output may overlap neither the extent of x, nor that of y, nor the window.  The launches allocate nothing and do not
 * synchronise, so they can be captured into a graph.
 *
 * Row contract: the bits of a group's outputs depend only on its T frames, the window and n -- not on the batch, the group's position
 * in it, the hop, the stream or the grid.  A NaN or Inf stays in the groups whose frames contain the sample.
 *
 * Return values: 0, a hipError_t, or -1 -- before any HIP call -- for n not one of the five lengths; T < 1; a negative count (streams,
 * groups); hop < 1; stream_stride < 1, x_stride < 1 or y_stride < 0; an extent or a count beyond 2^59 elements (computed in 128 bits);
 * grid < 1 (launch_tuned); a forbidden overlap.  A zero count launches nothing and returns 0.
 *
 * Out of scope:
 *   - detrend='constant' (scipy's default; subtract the mean first);
 *   - median averaging;
 *   - two-sided output;
 *   - n < 512, n > 8192 and n that is not a power of two;
 *   - a fused Pxx / Pyy / Pxy kernel for coherence (smfft_amd.welch.coherence makes three launches);
 *   - compensated or fp64 accumulation (the error grows like (T - 1) 2^-24; use a shorter T and sum the partial spectra);
 *   - cross spectra of all pairs of streams (a correlator).
 */
#ifndef SMFFT_WELCH_H_
#define SMFFT_WELCH_H_

#ifdef __cplusplus
extern "C" {
#endif

/* M = n / 2, the length of the complex transform inside the kernels, for n = 512 ... 8192 a power of two; -1 for every other n. */
int smfft_welch_fft_size(int n);

/* The whole groups of T frames of n samples at hop in a signal of L samples: floor(frames / T) with frames = 1 + (L - n) / hop (0 for
 * 0 <= L < n); -1 for an n that is not one of the five, hop < 1, T < 1 or L < 0. */
long long smfft_welch_groups(long long L, int n, long long hop, long long T);

/* streams * groups auto spectra of M + 1 float32 each, every one the sum of the powers of T frames of n float32 samples under the
 * window d_window (n floats, or NULL); enqueued on hip_stream (a hipStream_t; NULL = the null stream).  Launch only: no allocation, no
 * synchronisation. */
int smfft_welch_launch(const void* d_in, void* d_out, const void* d_window, int n, long long streams, long long groups, long long T, long long hop, long long stream_stride, void* hip_stream);

/* The same launch with the number of workgroups given (1 <= grid; the default is min(ceil(streams * groups * n / 8192), 12288),
 * grid-strided beyond).  The result does not depend on grid, to the bit. */
int smfft_welch_launch_tuned(const void* d_in, void* d_out, const void* d_window, int n, long long streams, long long groups, long long T, long long hop, long long stream_stride, void* hip_stream, int grid);

/* The same launch on the null stream, timed with events: ADDS the elapsed milliseconds to *FFT_time (when the launch was made and
 * FFT_time is not NULL) and returns after the kernel has finished. */
int smfft_welch_benchmark(const void* d_in, void* d_out, const void* d_window, int n, long long streams, long long groups, long long T, long long hop, long long stream_stride, double* FFT_time);

/* streams * groups cross spectra of M + 1 complex64 each: the sums of conj(X) Y over T frames of d_x and d_y. */
int smfft_csd_launch(const void* d_x, const void* d_y, void* d_out, const void* d_window, int n, long long streams, long long groups, long long T, long long hop, long long x_stride, long long y_stride, void* hip_stream);
int smfft_csd_launch_tuned(const void* d_x, const void* d_y, void* d_out, const void* d_window, int n, long long streams, long long groups, long long T, long long hop, long long x_stride, long long y_stride, void* hip_stream, int grid);
int smfft_csd_benchmark(const void* d_x, const void* d_y, void* d_out, const void* d_window, int n, long long streams, long long groups, long long T, long long hop, long long x_stride, long long y_stride, double* FFT_time);

#ifdef __cplusplus
}
#endif

#endif /* SMFFT_WELCH_H_ */

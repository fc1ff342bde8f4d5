/*
 * smfft_stft.h -- C ABI of libsmfft_stft.so: the batched short-time Fourier transform of real signals in frames of
 * n = 512, 1024, 2048, 4096 or 8192 samples at any hop, as complex spectra or as power (a spectrogram), and the inverse transform of
 * such frames, each in one kernel and one pass through HBM (one complex transform of M = n / 2 points of the register engine per
 * frame).  Overlapping frames are read from the signal itself: no framed copy is ever made.
 *
 * Definition.  Samples and window are float32, spectra complex64 (re, im interleaved).  All offsets are 64-bit.
 *   Forward:  X[k] = sum_{j<n} w[j] x[j] exp(-2 pi i jk / n),  k = 0 ... M  -- M + 1 = n / 2 + 1 bins, the one-sided spectrum of the
 *             windowed frame: np.fft.rfft(w x), torch.stft(..., center=False, onesided=True) transposed.
 *             kind 0 stores X[k] (complex64), kind 1 stores |X[k]|^2 = re*re + im*im (float32).
 *             The imaginary parts of X[0] and X[M] are exactly +0.
 *   Inverse:  y[j] = w[j] irfft_n(X)[j] = w[j] (1/n) sum_{k<n} X[k] exp(+2 pi i jk / n) with X[n-k] = conj X[k],  j < n.
 *             The imaginary parts of X[0] and X[M] are ignored (the C2R convention of torch.fft.irfft).  1/n is a power of two.
 * The window is a caller-supplied table of n floats on the device; NULL means all ones.
 *
 * Algorithm.  z[p] = w[2p] x[2p] + i w[2p+1] x[2p+1], p < M; Z = DFT_M(z); P[k] = conj Z[(M-k) mod M];
 * X[k] = (Z[k] + P[k]) / 2 - (i/2) W_n^k (Z[k] - P[k]), X[0] = Re Z[0] + Im Z[0], X[M] = Re Z[0] - Im Z[0].  The inverse runs the same
 * split backwards: A[k] = X[k], B[k] = conj X[M-k], Z'[k] = (A + B) + i conj(W_n^k) (A - B), z = the un-normalised inverse DFT_M(Z'),
 * y[2p] = w[2p] Re z[p] / n, y[2p+1] = w[2p+1] Im z[p] / n.  All twiddles are fp64 values rounded once to fp32.  One frame per
 * transform slot: 256 threads hold 8192 / n of them per workgroup; workgroups stride over the tiles.  There is no plan, no table to
 * prepare and no workspace.  
 *
 * Buffer contract: 4-byte alignment for the signal, the window and the float outputs, 8-byte alignment for complex rows; every output
 * element is written exactly once and nothing else is.
 *   stft:  frame (c, f), c < streams, f < frames, reads in[c*stream_stride + f*hop ... + n) and writes M + 1 values at element
 *          (c*frames + f)*(M + 1) of d_out: complex64 (kind 0) or float32 (kind 1).  Frames may overlap each other, hop may be any
 *          value >= 1, odd included; plain rows are frames = 1, stream_stride = n.  The output may overlap neither the input range
 *          in[0, (streams-1)*stream_stride + (frames-1)*hop + n) nor the window.
 *   istft: row r reads M + 1 complex64 at element r*(M + 1) and writes n floats at r*n, both contiguous; the output may overlap
 *          neither the input nor the window.  There is no overlap-add in the kernel.
 * The launches allocate nothing and do not synchronise, so they can be captured into a graph.
 *
 * Row contract: the bits of a frame's outputs depend only on that frame, the window, n and the kind -- not on the batch, the frame's
 * position in it, the hop, the stream or the grid.  A NaN or Inf stays in the frames that contain the sample.
 *
 * Return values: 0, a hipError_t, or -1 -- before any HIP call -- for n not one of the five lengths; a kind outside {0, 1}; a negative
 * count (streams, frames, batch); hop < 1 or stream_stride < 1; grid < 1 (launch_tuned); a forbidden overlap.  A zero count launches
 * nothing and returns 0.
 *
 * Out of scope:
 *   - center padding in the kernel (smfft_amd.stft pads in front of the launch);
 *   - two-sided output;
 *   - n < 512, n > 8192 and n that is not a power of two;
 *   - overlap-add inside the inverse kernel;
 *   - sums over frames (Welch);
 *   - any element type but float32 / complex64.
 */
#ifndef SMFFT_STFT_H_
#define SMFFT_STFT_H_

#ifdef __cplusplus
extern "C" {
#endif

/* M = n / 2, the length of the complex transform inside the kernels, for n = 512 ... 8192 a power of two; -1 for every other n. */
int smfft_stft_fft_size(int n);

/* The whole frames of n samples at hop in a signal of L samples: 1 + (L - n) / hop, 0 for 0 <= L < n; -1 for an n that is not one of
 * the five, hop < 1 or L < 0. */
long long smfft_stft_frames(long long L, int n, long long hop);

/* streams * frames transforms of frames of n float32 samples under the window d_window (n floats, or NULL), kind 0: M + 1 complex64
 * per frame, kind 1: M + 1 float32 powers per frame; enqueued on hip_stream (a hipStream_t; NULL = the null stream).  Launch only: no
 * allocation, no synchronisation. */
int smfft_stft_launch(const void* d_in, void* d_out, const void* d_window, int n, long long streams, long long frames, long long hop, long long stream_stride, int kind, void* hip_stream);

/* The same launch with the number of workgroups given (1 <= grid; the default is min(ceil(streams * frames * n / 8192), 12288),
 * grid-strided beyond).  The result does not depend on grid, to the bit. */
int smfft_stft_launch_tuned(const void* d_in, void* d_out, const void* d_window, int n, long long streams, long long frames, long long hop, long long stream_stride, int kind, void* hip_stream, int grid);

/* The same launch on the null stream, timed with events: ADDS the elapsed milliseconds to *FFT_time (when the launch was made and
 * FFT_time is not NULL) and returns after the kernel has finished. */
int smfft_stft_benchmark(const void* d_in, void* d_out, const void* d_window, int n, long long streams, long long frames, long long hop, long long stream_stride, int kind, double* FFT_time);

/* batch inverse transforms: rows of M + 1 complex64 in, rows of n windowed float32 samples out (d_window: n floats, or NULL). */
int smfft_istft_launch(const void* d_in, void* d_out, const void* d_window, int n, long long batch, void* hip_stream);
int smfft_istft_launch_tuned(const void* d_in, void* d_out, const void* d_window, int n, long long batch, void* hip_stream, int grid);
int smfft_istft_benchmark(const void* d_in, void* d_out, const void* d_window, int n, long long batch, double* FFT_time);

#ifdef __cplusplus
}
#endif

#endif /* SMFFT_STFT_H_ */

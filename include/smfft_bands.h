/*
 * smfft_bands.h -- C ABI of libsmfft_bands.so: band spectrograms (mel, Bark, octave bands, re-binning) of real signals.  The powers of
 * the frames of the short-time Fourier transform of smfft_stft.h (n = 512, 1024, 2048, 4096 or 8192 samples at any hop) are summed
 * along frequency into the bands of a prepared table inside the kernel, in one kernel and one pass through HBM: the frames' M + 1
 * powers never reach memory, and a launch stores `bands` values per frame.
 *
 * Definition.  Samples, window and weights are float32.  All offsets are 64-bit.  With M = n / 2, frame (c, f) reads
 * in[c*stream_stride + f*hop ... + n) under window[0, n) (NULL means all ones), and P[k] = re*re + im*im, k = 0 ... M, is the value
 * that smfft_stft_launch(kind = 1) stores for that frame, to the bit.
 *   A band table has `bands` bands, 1 <= bands <= M + 1.  Band b covers the consecutive bins first[b] ... first[b] + count[b] - 1 and
 *   carries count[b] float32 weights; 0 <= first[b], 0 <= count[b] and first[b] + count[b] <= M + 1.  The weights of all bands are
 *   concatenated in band order, weights = sum of count[b] <= 4 (M + 1).  Bands may overlap, be empty or have negative weights.
 *   Output, per frame:  out[(c*frames + f)*bands + b] = sum_i weight[b][i] * P[first[b] + i]          float32, written exactly once
 * An empty band stores exactly +0.  Each product is a statement of its own: t_i = weight[b][i] * P[first[b] + i], rounded to fp32.
 * Summation order: one thread per band, sequentially in ascending bin order, starting from -0: acc = -0, then acc = acc + t_i for
 * i = 0, 1, ... ((-0) + t_0 is t_0 to the bit).  It is fixed by the plan and n alone.  With the identity table (bands = M + 1,
 * first[b] = b, count[b] = 1, weight 1.0) the output equals smfft_stft_launch(kind = 1) bit for bit.
 *
 * Algorithm.  The frame-to-spectrum step of smfft_stft.h (windowed pairs in the two lanes of ONE complex transform of M points of the
 * register engine, partner through LDS, Hermitian split) and the power kind's statements; the M + 1 powers of a frame go as floats
 * into the transform slot's own LDS region, and thread u of the slot's n / 32 threads serves the bands u, u + n / 32, ...: it reads
 * first, count and offset of its band and the weights from the plan and stores one float per band, consecutive threads at consecutive
 * floats.  A plan of at most 11,264 words (45,056 bytes) is copied once per workgroup into LDS behind the transform regions and read
 * from there; a larger one is read from global memory per frame.  256 threads hold 8192 / n slots per workgroup; workgroups stride
 * over the tiles.  No workspace, no atomics, no transcendental and no allocation in a launch.  (INTEGRATION.md
 * section C20.)
 *
 * The plan: plan_bytes = 12*bands + 4*weights bytes on the device, 4-byte aligned: int32 first[bands], count[bands], offset[bands]
 * (the prefix sums of count: where a band's weights start), then the `weights` float32 weights.  The plan is written by
 * smfft_bands_tables / smfft_bands_prepare only: the launch cannot see the plan's contents and the kernel trusts it -- a plan that
 * did not come from them, or a launch with another n, bands or weights than the plan was made for, reads outside the plan or the
 * frame's powers.  A plan is read only and may serve any number of launches, concurrent ones included.
 *
 * Buffer contract: 4-byte alignment for the signal, the window, the plan and the output; every output element is written exactly once
 * and nothing else is.  The extent of the signal is in[0, (streams-1)*stream_stride + (frames-1)*hop + n).  The output may overlap
 * neither the extent of the signal, nor the window, nor the plan's plan_bytes.  The launches allocate nothing and do not synchronise,
 * so they can be captured into a graph.  smfft_bands_prepare copies from host memory and waits: it is not graph-capturable.
 *
 * Row contract: the bits of a frame's outputs depend only on the frame, the window, n and the plan -- not on the batch, the frame's
 * position in it, the hop, the stream or the grid.  A NaN or Inf stays in the frames that contain the sample (in the bands whose bins
 * it reaches: every band with at least one bin, since one sample reaches every bin of its frames).
 *
 * Return values: 0, a hipError_t, or -1 -- before any HIP call -- for n not one of the five lengths; bands outside 1 ... M + 1;
 * weights outside 0 ... 4 (M + 1); a NULL plan; a negative count (streams, frames); hop < 1; stream_stride < 1; an extent or a count
 * beyond 2^59 elements (computed in 128 bits); grid < 1 (launch_tuned); a forbidden overlap.  A zero count launches nothing and
 * returns 0.
 *
 * Out of scope:
 *   - log, dB or a DCT (MFCC) in the kernel (smfft_amd.bands.mel_spectrogram applies them in torch on the small output);
 *   - sums over frames combined with bands;
 *   - complex or magnitude (|X|, not |X|^2) band inputs;
 *   - dense matrices (a GEMM's job: weights is capped at 4 (M + 1));
 *   - n < 512, n > 8192 and n that is not a power of two.
 */
#ifndef SMFFT_BANDS_H_
#define SMFFT_BANDS_H_

#ifdef __cplusplus
extern "C" {
#endif

/* M = n / 2, the length of the complex transform inside the kernels, for n = 512 ... 8192 a power of two; -1 for every other n. */
int smfft_bands_fft_size(int n);

/* The whole frames of n samples at hop in a signal of L samples: 1 + (L - n) / hop (0 for 0 <= L < n), as smfft_stft_frames; -1 for
 * an n that is not one of the five, hop < 1 or L < 0. */
long long smfft_bands_frames(long long L, int n, long long hop);

/* The bytes of the plan of a table of `bands` bands with `weights` weights in all: 12*bands + 4*weights; -1 for an n that is not one
 * of the five, bands outside 1 ... M + 1 or weights outside 0 ... 4 (M + 1). */
long long smfft_bands_plan_bytes(int n, int bands, int weights);

/* Host only, no HIP call: checks the table (h_first and h_count: `bands` int32 each; h_weights: the sum of h_count floats, in band
 * order; it may be NULL where that sum is 0) against every rule of the definition and writes its plan, smfft_bands_plan_bytes(n,
 * bands, sum of h_count) bytes, to h_plan.  0, or -1 for a violation (and nothing is written). */
int smfft_bands_tables(int n, int bands, const void* h_first, const void* h_count, const void* h_weights, void* h_plan);

/* The same check, then the plan is built on the host, copied to d_plan on hip_stream and waited for: when the call returns, the plan
 * is in place and no host memory is in use.  Not graph-capturable. */
int smfft_bands_prepare(int n, int bands, const void* h_first, const void* h_count, const void* h_weights, void* d_plan, void* hip_stream);

/* streams * frames rows of `bands` float32 each: the band sums of the powers of every frame of n float32 samples under the window
 * d_window (n floats, or NULL) with the plan d_plan of a table of `bands` bands and `weights` weights; enqueued on hip_stream (a
 * hipStream_t; NULL = the null stream).  Launch only: no allocation, no synchronisation. */
int smfft_bands_launch(const void* d_in, void* d_out, const void* d_window, const void* d_plan, int n, int bands, int weights, long long streams, long long frames, long long hop, long long stream_stride, void* hip_stream);

/* The same launch with the number of workgroups given (1 <= grid; the default is min(ceil(streams * frames * n / 8192), 12288),
 * grid-strided beyond).  The result does not depend on grid, to the bit. */
int smfft_bands_launch_tuned(const void* d_in, void* d_out, const void* d_window, const void* d_plan, int n, int bands, int weights, long long streams, long long frames, long long hop, long long stream_stride, void* hip_stream, int grid);

/* The same launch on the null stream, timed with events: ADDS the elapsed milliseconds to *FFT_time (when the launch was made and
 * FFT_time is not NULL) and returns after the kernel has finished. */
int smfft_bands_benchmark(const void* d_in, void* d_out, const void* d_window, const void* d_plan, int n, int bands, int weights, long long streams, long long frames, long long hop, long long stream_stride, double* FFT_time);

#ifdef __cplusplus
}
#endif

#endif /* SMFFT_BANDS_H_ */

/*
 * smfft_large.h -- C ABI of libsmfft_large.so: batched C2C FFTs of N = 8192 and 16384 in one pass through HBM.
 *
 * A library of its own, beside libsmfft_amd.so: smfft_launch, the c2c calls and the reference API keep answering
 * "wrong FFT length" above N = 4096.  Each FFT is transformed whole in one workgroup's LDS (gfx950: 160 KiB per CU): one read
 * of the input, one write of the output (include/smfft/smfft_large.hpp).
 *
 * Conventions (those of include/smfft.h):
 *   - complex data is interleaved float (re, im) = float2; FFT f of a batch is at element f*N (64-bit offsets);
 *   - natural order in and out, un-normalised; inverse = 0: X[k] = sum x[n] e^{-2 pi i nk/N}, inverse != 0: the + sign
 *     (the signs of smfft_ct_external_benchmark with reorder = 1); inverse(forward(x)) = N x;
 *   - buffer contract: pointers 8-byte aligned (interior pointers are fine); only FFTs [0, nFFTs) of either buffer are read or
 *     written; d_output == d_input is allowed, partial overlap is not; the input is left untouched unless it is the output.
 */
#ifndef SMFFT_LARGE_H_
#define SMFFT_LARGE_H_

#ifdef __cplusplus
extern "C" {
#endif

/* d_output[f] = FFT(d_input[f]), f < nFFTs, enqueued on hip_stream (a hipStream_t; NULL = the null stream).  Launch only: no
 * synchronisation.  Returns 0, a hipError_t of the launch, or -1 -- before any HIP call -- for FFT_size not 8192 / 16384 or
 * nFFTs < 0.  nFFTs = 0 launches nothing. */
int smfft_large_launch(const void* d_input, void* d_output, int FFT_size, int nFFTs, int inverse, void* hip_stream);

/* The same launch on the null stream, timed with events: ADDS the elapsed milliseconds to *FFT_time (when the launch was made
 * and FFT_time is not NULL) and returns after the kernel has finished.  Same return values. */
int smfft_large_benchmark(const void* d_input, void* d_output, int FFT_size, int nFFTs, int inverse, double* FFT_time);

/* The persistent grid a launch of FFT_size uses on the current device when nFFTs is at least as large (workgroups: one per CU at
 * 16384, two at 8192); -1 for an unsupported FFT_size (before any HIP call), 0 when the device cannot be queried. */
int smfft_large_grid(int FFT_size);

#ifdef __cplusplus
}
#endif

#endif /* SMFFT_LARGE_H_ */

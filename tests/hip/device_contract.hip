// device_contract.hip -- test kernels for the header-only device API (include/smfft_device.hpp) that the library's own kernels do
// not reach: user kernels written the way upstream's users write them (blockDim.x = fft_length / 4, the reference's grid arithmetic),
// around do_FFT_Stockham_mk6 / _C2C / _R2C_C2R, the registers forms, the two-argument kernels of N = 32 ... 128, chains with a runtime
// count, the smfft::tiled functions (do_SMFFT_CT_DIT among them) and -- in the -DNREUSES=3 build -- the header's `multiple` kernels.  tests/test_device_contract_gpu.py
// compares every one of them with fp64.  Built by smfft_amd/csrc/Makefile (libsmfft_device_contract*.so), never shipped.
//
// LDS canaries: a launcher given a non-null `canary` counter allocates the function's documented footprint plus kCanary float2, fills
// the extra words with a bit pattern before the call and adds the number of changed words to *canary after the drain.  With a null
// counter the allocation is exactly the footprint.
#include <hip/hip_runtime.h>
#include <smfft_device.hpp>

namespace {

constexpr int kCanary = 64;
constexpr unsigned kPattern = 0x7FA5C3E1u;     // a NaN no transform produces from finite data

__device__ __forceinline__ void canary_fill(float2* s, int footprint, const int* canary) {
    if (!canary) return;
    for (int i = threadIdx.x; i < kCanary; i += blockDim.x) s[footprint + i] = make_float2(__uint_as_float(kPattern), __uint_as_float(~kPattern));
}
// (behind a barrier of its own: the function's writes, wherever they went, are all done)
__device__ __forceinline__ void canary_check(const float2* s, int footprint, int* canary) {
    if (!canary) return;
    __syncthreads();
    int changed = 0;
    for (int i = threadIdx.x; i < kCanary; i += blockDim.x) {
        const float2 v = s[footprint + i];
        changed += (__float_as_uint(v.x) != kPattern || __float_as_uint(v.y) != ~kPattern) ? 1 : 0;
    }
    if (changed) atomicAdd(canary, changed);
}
__host__ __device__ constexpr size_t lds_bytes(int footprint, const int* canary) { return (size_t)(footprint + (canary ? kCanary : 0)) * sizeof(float2); }

// ------------------------------------------------------------------------------------------------
// fill / call / drain in the reference's shape: one block of N / 4 threads per transform, drained RIGHT AFTER the call (ST:253,
// RC:360-361: the functions end with a barrier).  FN: 0 do_FFT_Stockham_mk6 (N float2), 1 / 2 do_FFT_Stockham_C2C forward / inverse
// (L + 1), 3 / 4 do_FFT_Stockham_R2C_C2R forward / inverse (L + 1).
// ------------------------------------------------------------------------------------------------
template <class P, int FN>
__global__ void st_fill_call_drain(const float2* d_input, float2* d_output, int* canary) {
    extern __shared__ float2 s_dynamic[];
    float2* s = s_dynamic;
    constexpr int footprint = FN == 0 ? P::fft_length : P::fft_length + 1;
    const int base = threadIdx.x + blockIdx.x * P::fft_length;
    for (int k = 0; k < 4; k++) s[threadIdx.x + k * P::fft_quarter] = d_input[base + k * P::fft_quarter];
    canary_fill(s, footprint, canary);
    __syncthreads();
    if constexpr (FN == 0) do_FFT_Stockham_mk6<P>(s);
    else if constexpr (FN == 1) do_FFT_Stockham_C2C<P, FFT_forward>(s);
    else if constexpr (FN == 2) do_FFT_Stockham_C2C<P, FFT_inverse>(s);
    else if constexpr (FN == 3) do_FFT_Stockham_R2C_C2R<P, FFT_forward>(s);
    else do_FFT_Stockham_R2C_C2R<P, FFT_inverse>(s);
    for (int k = 0; k < 4; k++) d_output[base + k * P::fft_quarter] = s[threadIdx.x + k * P::fft_quarter];
    canary_check(s, footprint, canary);
}

// chains with a count the compiler cannot unroll: FN 1: do_FFT_Stockham_C2C forward then inverse (N x per round), 3: R2C then C2R on
// the same LDS array (L x per round)
template <class P, int FN>
__global__ void st_chain(const float2* d_input, float2* d_output, int rounds) {
    extern __shared__ float2 s_dynamic[];
    float2* s = s_dynamic;
    const int base = threadIdx.x + blockIdx.x * P::fft_length;
    for (int k = 0; k < 4; k++) s[threadIdx.x + k * P::fft_quarter] = d_input[base + k * P::fft_quarter];
    __syncthreads();
    for (int r = 0; r < rounds; r++) {
        if constexpr (FN == 1) {
            do_FFT_Stockham_C2C<P, FFT_forward>(s);
            do_FFT_Stockham_C2C<P, FFT_inverse>(s);
        } else {
            do_FFT_Stockham_R2C_C2R<P, FFT_forward>(s);
            do_FFT_Stockham_R2C_C2R<P, FFT_inverse>(s);
        }
    }
    for (int k = 0; k < 4; k++) d_output[base + k * P::fft_quarter] = s[threadIdx.x + k * P::fft_quarter];
}

// ------------------------------------------------------------------------------------------------
// registers forms, inputs loaded as INTEGRATION.md's snippet does (natural order: element t + m N/4; no reorder: 4 t + m).
// FN: 0 do_FFT_Stockham_C2C_registers<P, D>, 1 do_FFT_Stockham_C2C_registers_out<P, D> (scratch: N float2, as FFT_GPU_external
// passes it), 2 do_SMFFT_CT_DIT_registers<P> (P a CT class, D ignored; scratch: P::fft_sm_required, as SMFFT_DIT_external).
// ------------------------------------------------------------------------------------------------
template <class P, int FN, class D>
__global__ void registers_kernel(const float2* d_input, float2* d_output, int* canary) {
    extern __shared__ float2 s_dynamic[];
    float2* s = s_dynamic;
    constexpr int N = P::fft_length;
    constexpr int Q = N / 4;
    int footprint = N;
    bool natural = true;
    if constexpr (FN == 2) footprint = P::fft_sm_required, natural = P::fft_reorder != 0;
    const size_t block = (size_t)blockIdx.x * N;
    canary_fill(s, footprint, canary);
    if (canary) __syncthreads();
    float2 x[4];
    for (int m = 0; m < 4; m++) x[m] = d_input[block + (natural ? threadIdx.x + m * Q : 4 * threadIdx.x + m)];
    int element[4] = {(int)threadIdx.x, (int)threadIdx.x + Q, (int)threadIdx.x + 2 * Q, (int)threadIdx.x + 3 * Q};
    if constexpr (FN == 0) do_FFT_Stockham_C2C_registers<P, D>(x, s);
    else if constexpr (FN == 1) do_FFT_Stockham_C2C_registers_out<P, D>(x, s, element);
    else do_SMFFT_CT_DIT_registers<P>(x, s);
    for (int m = 0; m < 4; m++) d_output[block + element[m]] = x[m];
    canary_check(s, footprint, canary);
}

// ------------------------------------------------------------------------------------------------
// the tiled contract: 256 threads, 4096 / N transforms per workgroup at a stride of smfft::Geometry<N>::SF = 17 N / 16, in an LDS
// array of 4352 float2.  FN as st_fill_call_drain; 5: smfft::tiled::do_SMFFT_CT_DIT<P> (P a CT class, N = P::fft_size).
// ------------------------------------------------------------------------------------------------
template <class P, int FN, int N = P::fft_length>
__global__ void tiled_kernel(const float2* d_input, float2* d_output, int* canary) {
    extern __shared__ float2 s_dynamic[];
    float2* s = s_dynamic;
    constexpr int SF = smfft::Geometry<N>::SF, footprint = 4352;
    const size_t block = (size_t)blockIdx.x * 4096;
    for (int i = threadIdx.x; i < 4096; i += 256) s[(i / N) * SF + i % N] = d_input[block + i];
    canary_fill(s, footprint, canary);
    __syncthreads();
    if constexpr (FN == 0) smfft::tiled::do_FFT_Stockham_mk6<P>(s);
    else if constexpr (FN == 1) smfft::tiled::do_FFT_Stockham_C2C<P, FFT_forward>(s);
    else if constexpr (FN == 2) smfft::tiled::do_FFT_Stockham_C2C<P, FFT_inverse>(s);
    else if constexpr (FN == 3) smfft::tiled::do_FFT_Stockham_R2C_C2R<P, FFT_forward>(s);
    else if constexpr (FN == 4) smfft::tiled::do_FFT_Stockham_R2C_C2R<P, FFT_inverse>(s);
    else smfft::tiled::do_SMFFT_CT_DIT<P>(s);
    __syncthreads();
    for (int i = threadIdx.x; i < 4096; i += 256) d_output[block + i] = s[(i / N) * SF + i % N];
    canary_check(s, footprint, canary);
}

template <class P>
int launch_st(int fn, const float2* in, float2* out, int nFFTs, int* canary, hipStream_t st) {
    const int footprint = fn == 0 ? P::fft_length : P::fft_length + 1;
    const size_t lds = lds_bytes(footprint, canary);
    const dim3 grid(nFFTs), block(P::fft_length / 4);
    switch (fn) {
        case 0: st_fill_call_drain<P, 0><<<grid, block, lds, st>>>(in, out, canary); break;
        case 1: st_fill_call_drain<P, 1><<<grid, block, lds, st>>>(in, out, canary); break;
        case 2: st_fill_call_drain<P, 2><<<grid, block, lds, st>>>(in, out, canary); break;
        case 3: if constexpr (P::fft_length <= 2048) { st_fill_call_drain<P, 3><<<grid, block, lds, st>>>(in, out, canary); break; } else return -1;
        case 4: if constexpr (P::fft_length <= 2048) { st_fill_call_drain<P, 4><<<grid, block, lds, st>>>(in, out, canary); break; } else return -1;
        default: return -1;
    }
    return (int)hipGetLastError();
}

template <class P>
int launch_chain(int fn, const float2* in, float2* out, int nFFTs, int rounds, hipStream_t st) {
    const size_t lds = (size_t)(P::fft_length + 1) * sizeof(float2);
    if (fn == 1) st_chain<P, 1><<<dim3(nFFTs), dim3(P::fft_length / 4), lds, st>>>(in, out, rounds);
    else if constexpr (P::fft_length <= 2048) {
        if (fn == 3) st_chain<P, 3><<<dim3(nFFTs), dim3(P::fft_length / 4), lds, st>>>(in, out, rounds);
        else return -1;
    } else return -1;
    return (int)hipGetLastError();
}

template <class P>
int launch_tiled(int fn, const float2* in, float2* out, int nFFTs, int* canary, hipStream_t st) {
    const int per = 4096 / P::fft_length;
    if (nFFTs % per) return -1;
    const size_t lds = lds_bytes(4352, canary);
    const dim3 grid(nFFTs / per), block(256);
    switch (fn) {
        case 0: tiled_kernel<P, 0><<<grid, block, lds, st>>>(in, out, canary); break;
        case 1: tiled_kernel<P, 1><<<grid, block, lds, st>>>(in, out, canary); break;
        case 2: tiled_kernel<P, 2><<<grid, block, lds, st>>>(in, out, canary); break;
        case 3: if constexpr (P::fft_length <= 2048) { tiled_kernel<P, 3><<<grid, block, lds, st>>>(in, out, canary); break; } else return -1;
        case 4: if constexpr (P::fft_length <= 2048) { tiled_kernel<P, 4><<<grid, block, lds, st>>>(in, out, canary); break; } else return -1;
        default: return -1;
    }
    return (int)hipGetLastError();
}

template <class P>
int launch_tiled_ct(const float2* in, float2* out, int nFFTs, int* canary, hipStream_t st) {
    constexpr int N = P::fft_size;
    if (nFFTs % (4096 / N)) return -1;
    tiled_kernel<P, 5, N><<<dim3(nFFTs / (4096 / N)), dim3(256), lds_bytes(4352, canary), st>>>(in, out, canary);
    return (int)hipGetLastError();
}

template <class P>
int launch_st_registers(int fn, int inverse, const float2* in, float2* out, int nFFTs, int* canary, hipStream_t st) {
    const size_t lds = lds_bytes(P::fft_length, canary);
    const dim3 grid(nFFTs), block(P::fft_length / 4);
    if (fn == 0 && !inverse) registers_kernel<P, 0, FFT_forward><<<grid, block, lds, st>>>(in, out, canary);
    else if (fn == 0) registers_kernel<P, 0, FFT_inverse><<<grid, block, lds, st>>>(in, out, canary);
    else if (fn == 1 && !inverse) registers_kernel<P, 1, FFT_forward><<<grid, block, lds, st>>>(in, out, canary);
    else if (fn == 1) registers_kernel<P, 1, FFT_inverse><<<grid, block, lds, st>>>(in, out, canary);
    else return -1;
    return (int)hipGetLastError();
}

template <class P>
int launch_ct_registers(const float2* in, float2* out, int nFFTs, int* canary, hipStream_t st) {
    registers_kernel<P, 2, FFT_forward><<<dim3(nFFTs), dim3(P::fft_length / 4), lds_bytes(P::fft_sm_required, canary), st>>>(in, out, canary);
    return (int)hipGetLastError();
}

}  // namespace

#define DC_ST_SIZES(X) X(32) X(64) X(128) X(256) X(512) X(1024) X(2048) X(4096)

// fn: 0 do_FFT_Stockham_mk6, 1 / 2 do_FFT_Stockham_C2C forward / inverse, 3 / 4 do_FFT_Stockham_R2C_C2R forward / inverse (N = L)
extern "C" int dc_stockham(int fn, const void* in, void* out, int N, int nFFTs, int* canary, void* stream) {
    const float2* i = (const float2*)in;
    float2* o = (float2*)out;
    hipStream_t st = (hipStream_t)stream;
#define X(n) case n: return launch_st<FFT_##n>(fn, i, o, nFFTs, canary, st);
    switch (N) { DC_ST_SIZES(X) default: return -1; }
#undef X
}

// fn: 1 Stockham forward + inverse per round, 3 R2C + C2R per round
extern "C" int dc_chain(int fn, const void* in, void* out, int N, int nFFTs, int rounds, void* stream) {
    const float2* i = (const float2*)in;
    float2* o = (float2*)out;
    hipStream_t st = (hipStream_t)stream;
#define X(n) case n: return launch_chain<FFT_##n>(fn, i, o, nFFTs, rounds, st);
    switch (N) { DC_ST_SIZES(X) default: return -1; }
#undef X
}

// fn as dc_stockham, smfft::tiled:: functions; nFFTs a multiple of 4096 / N
extern "C" int dc_tiled(int fn, const void* in, void* out, int N, int nFFTs, int* canary, void* stream) {
    const float2* i = (const float2*)in;
    float2* o = (float2*)out;
    hipStream_t st = (hipStream_t)stream;
#define X(n) case n: return launch_tiled<FFT_##n>(fn, i, o, nFFTs, canary, st);
    switch (N) { DC_ST_SIZES(X) default: return -1; }
#undef X
}

// smfft::tiled::do_SMFFT_CT_DIT<FFT_<N>_{forward,inverse}{,_noreorder}>, N = 32 ... 4096; nFFTs a multiple of 4096 / N
extern "C" int dc_tiled_ct(int inverse, int reorder, const void* in, void* out, int N, int nFFTs, int* canary, void* stream) {
    const float2* i = (const float2*)in;
    float2* o = (float2*)out;
    hipStream_t st = (hipStream_t)stream;
#define X(n)                                                                                                   \
    case n:                                                                                                    \
        if (!inverse && reorder) return launch_tiled_ct<FFT_##n##_forward>(i, o, nFFTs, canary, st);          \
        if (!inverse) return launch_tiled_ct<FFT_##n##_forward_noreorder>(i, o, nFFTs, canary, st);           \
        if (reorder) return launch_tiled_ct<FFT_##n##_inverse>(i, o, nFFTs, canary, st);                      \
        return launch_tiled_ct<FFT_##n##_inverse_noreorder>(i, o, nFFTs, canary, st);
    switch (N) { DC_ST_SIZES(X) default: return -1; }
#undef X
}

// fn: 0 do_FFT_Stockham_C2C_registers, 1 do_FFT_Stockham_C2C_registers_out
extern "C" int dc_stockham_registers(int fn, int inverse, const void* in, void* out, int N, int nFFTs, int* canary, void* stream) {
    const float2* i = (const float2*)in;
    float2* o = (float2*)out;
    hipStream_t st = (hipStream_t)stream;
#define X(n) case n: return launch_st_registers<FFT_##n>(fn, inverse, i, o, nFFTs, canary, st);
    switch (N) { DC_ST_SIZES(X) default: return -1; }
#undef X
}

// do_SMFFT_CT_DIT_registers<FFT_<N>_{forward,inverse}{,_noreorder}>, N >= 256
extern "C" int dc_ct_registers(int inverse, int reorder, const void* in, void* out, int N, int nFFTs, int* canary, void* stream) {
    const float2* i = (const float2*)in;
    float2* o = (float2*)out;
    hipStream_t st = (hipStream_t)stream;
#define X(n)                                                                                                   \
    case n:                                                                                                    \
        if (!inverse && reorder) return launch_ct_registers<FFT_##n##_forward>(i, o, nFFTs, canary, st);      \
        if (!inverse) return launch_ct_registers<FFT_##n##_forward_noreorder>(i, o, nFFTs, canary, st);       \
        if (reorder) return launch_ct_registers<FFT_##n##_inverse>(i, o, nFFTs, canary, st);                  \
        return launch_ct_registers<FFT_##n##_inverse_noreorder>(i, o, nFFTs, canary, st);
    switch (N) { X(256) X(512) X(1024) X(2048) X(4096) default: return -1; }
#undef X
}

// the header's two-argument Stockham kernel at the lengths upstream does not have: FFT_GPU_external<FFT_N><<<nFFTs, N/4, N*8>>>
extern "C" int dc_fft_gpu_external(const void* in, void* out, int N, int nFFTs, void* stream) {
    float2* i = (float2*)in;
    float2* o = (float2*)out;
    hipStream_t st = (hipStream_t)stream;
    switch (N) {
        case 32: FFT_GPU_external<FFT_32><<<dim3(nFFTs), dim3(8), 32 * 8, st>>>(i, o); break;
        case 64: FFT_GPU_external<FFT_64><<<dim3(nFFTs), dim3(16), 64 * 8, st>>>(i, o); break;
        case 128: FFT_GPU_external<FFT_128><<<dim3(nFFTs), dim3(32), 128 * 8, st>>>(i, o); break;
        default: return -1;
    }
    return (int)hipGetLastError();
}

// the header's `multiple` kernels (NREUSES applications; the -DNREUSES=3 build makes them checkable), in the reference's launch shapes
extern "C" int dc_nreuses() { return NREUSES; }

template <class P>
static int launch_ct_multiple(float2* in, float2* out, int nFFTs, hipStream_t st) {
    const int per = P::fft_length / P::fft_size;
    if (nFFTs % per) return -1;
    SMFFT_DIT_multiple<P><<<dim3(nFFTs / per), dim3(P::fft_length / 4), 0, st>>>(in, out);
    return (int)hipGetLastError();
}
// wave64: the FFT_<N>_..._wave64 classes (N <= 128)
extern "C" int dc_ct_multiple(int inverse, int reorder, int wave64, const void* in, void* out, int N, int nFFTs, void* stream) {
    float2* i = (float2*)in;
    float2* o = (float2*)out;
    hipStream_t st = (hipStream_t)stream;
#define CLASSES(n, SUF)                                                                                            \
    if (!inverse && reorder) return launch_ct_multiple<FFT_##n##_forward##SUF>(i, o, nFFTs, st);                  \
    if (!inverse) return launch_ct_multiple<FFT_##n##_forward_noreorder##SUF>(i, o, nFFTs, st);                   \
    if (reorder) return launch_ct_multiple<FFT_##n##_inverse##SUF>(i, o, nFFTs, st);                              \
    return launch_ct_multiple<FFT_##n##_inverse_noreorder##SUF>(i, o, nFFTs, st);
#define X(n) case n: if (wave64) { CLASSES(n, _wave64) } CLASSES(n, )
#define Y(n) case n: if (wave64) return -1; CLASSES(n, )
    switch (N) { X(32) X(64) X(128) Y(256) Y(512) Y(1024) Y(2048) Y(4096) default: return -1; }
#undef X
#undef Y
#undef CLASSES
}

extern "C" int dc_fft_gpu_multiple(const void* in, void* out, int N, int nFFTs, void* stream) {
    float2* i = (float2*)in;
    float2* o = (float2*)out;
    hipStream_t st = (hipStream_t)stream;
#define X(n) case n: FFT_GPU_multiple<FFT_##n><<<dim3(nFFTs), dim3(n / 4), n * 8, st>>>(i, o); break;
    switch (N) { DC_ST_SIZES(X) default: return -1; }
#undef X
    return (int)hipGetLastError();
}

extern "C" int dc_rc_multiple(int inverse, const void* in, void* out, int L, int nFFTs, void* stream) {
    float2* i = (float2*)in;
    float2* o = (float2*)out;
    hipStream_t st = (hipStream_t)stream;
#define X(n)                                                                                                                         \
    case n:                                                                                                                          \
        if (inverse) FFT_GPU_R2C_C2R_multiple<FFT_##n, FFT_inverse><<<dim3(nFFTs), dim3(n / 4), 0, st>>>(i, o);                     \
        else FFT_GPU_R2C_C2R_multiple<FFT_##n, FFT_forward><<<dim3(nFFTs), dim3(n / 4), 0, st>>>(i, o);                             \
        break;
    switch (L) { X(32) X(64) X(128) X(256) X(512) X(1024) X(2048) default: return -1; }
#undef X
    return (int)hipGetLastError();
}

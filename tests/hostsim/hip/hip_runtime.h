// hip/hip_runtime.h -- a stand-in for the HIP runtime header, for HOST-ONLY compiles of barrier-synchronised kernels
// (tests/hostsim/README.md).  Put tests/hostsim first on the include path and compile as plain C++17 with clang (the
// headers use address_space(1) and ext_vector_type).  A kernel thread is a fiber of the executor (hostsim.hpp): exactly one runs
// at a time, so threadIdx / blockIdx and the `static` image behind __shared__ are plain globals that the executor sets before
// it resumes a thread.
//
// What a large kernel (include/smfft/smfft_large*.hpp) reaches is modelled; what it does not reach but its headers mention
// (lane permutes, buffer loads, wave-level fences, hardware registers) ABORTS WITH ITS NAME when executed: a stand-in never
// returns a value silently.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define __host__
#define __device__
#define __global__
#define __forceinline__ inline __attribute__((always_inline))
#define __launch_bounds__(...)
#define __restrict__ __restrict
// __attribute__((amdgpu_waves_per_eu(n))) applies to device kernels only: an attribute without effect in its place
#define amdgpu_waves_per_eu(...) unused

// ---- vector types and index variables -----------------------------------------------------------------------------------
struct alignas(8) float2 { float x, y; };
static inline float2 make_float2(float x, float y) { return float2{x, y}; }
struct uint3 { unsigned x, y, z; };
struct dim3 {
    unsigned x, y, z;
    constexpr dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};

namespace hostsim {
extern uint3 thread_idx, block_idx;      // of the kernel thread that is running
extern dim3 block_dim, grid_dim;
void barrier();                          // __syncthreads(): back to the executor until the workgroup's interval is over
[[noreturn]] void unmodelled(const char* what, const char* where);
void asm_statement(const char* text, const char* where);
template <class T>
T unmodelled_value(const char* what, const char* where) { unmodelled(what, where); }
}  // namespace hostsim

#define threadIdx (::hostsim::thread_idx)
#define blockIdx (::hostsim::block_idx)
#define blockDim (::hostsim::block_dim)
#define gridDim (::hostsim::grid_dim)

// One image per RUNNING workgroup: workgroups run one after another, so a kernel's __shared__ array is a static of its own.
// All of them live in one section, each on a 1 MiB boundary: the executor fills the whole section with its prefill pattern before
// a workgroup starts, finds the image of the running kernel by the first bytes that changed, and treats the padding between the
// images as guard bands (hostsim.cpp).
#define HOSTSIM_LDS_ALIGN (1 << 20)
#define __shared__ static __attribute__((section("hostsim_lds"), aligned(HOSTSIM_LDS_ALIGN)))
#define __syncthreads() ::hostsim::barrier()

// ---- asm statements ---------------------------------------------------------------------------------------------------
// `asm volatile(TEXT : OUT : IN : CLOBBER)` cannot be given to a host assembler.  `asm` expands to nothing and `volatile(...)` --
// the qualifier `volatile` is never followed by a parenthesis elsewhere -- to a call that receives the statement as a string:
// an EMPTY instruction string (an optimisation barrier such as LargeEngine::reload_twiddles()) is inert, any other aborts.
#define asm
#define volatile(...) ::hostsim::asm_statement(#__VA_ARGS__, __func__)

// ---- plain functions of the HIP headers ---------------------------------------------------------------------------------
static inline unsigned __float_as_uint(float v) { unsigned u; std::memcpy(&u, &v, 4); return u; }
static inline int __float_as_int(float v) { int u; std::memcpy(&u, &v, 4); return u; }
static inline float __uint_as_float(unsigned u) { float v; std::memcpy(&v, &u, 4); return v; }
static inline float __int_as_float(int u) { float v; std::memcpy(&v, &u, 4); return v; }
static inline unsigned __brev(unsigned v) {
    unsigned r = 0;
    for (int i = 0; i < 32; ++i) r |= ((v >> i) & 1u) << (31 - i);
    return r;
}

// ---- gfx950-only builtins and types: not reached by the large kernels ----------------------------------------------------
struct __amdgpu_buffer_rsrc_t { const void* base; };
typedef unsigned hostsim_uint2v __attribute__((ext_vector_type(2)));
typedef unsigned hostsim_uint4v __attribute__((ext_vector_type(4)));
#define HOSTSIM_UNMODELLED(T, name) (::hostsim::unmodelled_value<T>(name, __func__))
#define __builtin_amdgcn_make_buffer_rsrc(...) HOSTSIM_UNMODELLED(__amdgpu_buffer_rsrc_t, "__builtin_amdgcn_make_buffer_rsrc")
#define __builtin_amdgcn_raw_buffer_load_b128(...) HOSTSIM_UNMODELLED(hostsim_uint4v, "__builtin_amdgcn_raw_buffer_load_b128")
#define __builtin_amdgcn_raw_buffer_store_b128(...) HOSTSIM_UNMODELLED(int, "__builtin_amdgcn_raw_buffer_store_b128")
#define __builtin_amdgcn_permlane16_swap(...) HOSTSIM_UNMODELLED(hostsim_uint2v, "__builtin_amdgcn_permlane16_swap")
#define __builtin_amdgcn_permlane32_swap(...) HOSTSIM_UNMODELLED(hostsim_uint2v, "__builtin_amdgcn_permlane32_swap")
#define __builtin_amdgcn_update_dpp(...) HOSTSIM_UNMODELLED(int, "__builtin_amdgcn_update_dpp")
#define __builtin_amdgcn_ds_swizzle(...) HOSTSIM_UNMODELLED(int, "__builtin_amdgcn_ds_swizzle")
#define __builtin_amdgcn_s_getreg(...) HOSTSIM_UNMODELLED(unsigned, "__builtin_amdgcn_s_getreg")
#define __builtin_amdgcn_s_setprio(...) HOSTSIM_UNMODELLED(int, "__builtin_amdgcn_s_setprio")
// the synchronisation of an FFT that lives inside one wave (fft_sync<false>): instruction order within a wave, which this
// executor does not model
#define __builtin_amdgcn_fence(...) HOSTSIM_UNMODELLED(int, "__builtin_amdgcn_fence")
#define __builtin_amdgcn_wave_barrier() HOSTSIM_UNMODELLED(int, "__builtin_amdgcn_wave_barrier")

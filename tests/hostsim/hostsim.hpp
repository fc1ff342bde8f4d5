// hostsim.hpp -- a host executor for barrier-synchronised kernels (tests/hostsim/README.md).
//
// It runs a __global__ function, compiled as plain C++ against tests/hostsim/hip/hip_runtime.h, over a grid of workgroups.  It
// knows threads, __syncthreads(), one LDS image per running workgroup and a SCHEDULE; it is not a GPU simulator.  Kernel threads
// are fibers and exactly one runs at a time: a barrier interval of a workgroup (from one __syncthreads() to the next, or to the
// kernel's end) is executed thread by thread, each thread from its barrier to its next one, in the order the schedule chooses.
// A run is therefore a deterministic function of (kernel, inputs, schedule, seed), and two threads that touch the same LDS slot
// in one interval without a barrier between them give different results under the two schedules that order them differently.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

namespace hostsim {

enum Schedule {
    kAscending = 0,       // threads 0, 1, ... T-1 in every interval
    kDescending = 1,      // T-1 ... 0: with kAscending, every pair of threads runs in both orders in every interval
    kWaves = 2,           // 64-thread waves in a fresh seeded permutation per interval, lanes ascending
    kRandom = 3,          // a fresh seeded permutation of all T threads per interval
};

enum Error {
    kOk = 0,
    kDivergentBarrier = 1,     // threads of one workgroup reached different numbers of barriers (or part of it returned early)
    kLdsOutOfBounds = 2,       // a write outside the running kernel's __shared__ image
    kGlobalOutOfBounds = 3,    // a write into the guard band of a watched global buffer
    kBadLaunch = 4,
};

// the LDS prefill: a signalling NaN with a payload of its own, in every 32-bit word of the image before a workgroup starts
constexpr uint32_t kLdsPrefill = 0x7fa5c0deu;

struct Config {
    int grid = 1, threads = 1;
    int schedule = kAscending;
    uint64_t seed = 0;
    bool blocks_descending = false;      // workgroups run one after another, first to last or last to first
    // barrier knock-out (a property of the host run only): with period P > 0, every thread's barriers number k, k + P, k + 2P ...
    // are treated as absent -- the thread runs straight through into the next interval
    int knock_out = -1, period = 0;
    size_t lds_bytes = 0;                // size of the kernel's __shared__ array (0: it has none)
};

// a global buffer with `guard` bytes on either side that no kernel thread may change
struct Watch {
    const void* base;
    size_t bytes, guard;
};

struct Result {
    int error = kOk;
    std::string message;
    std::vector<long> barriers;          // per workgroup (blockIdx.x): __syncthreads() calls of each of its threads, knocked-out ones included
};

Result run(const Config& cfg, const std::function<void()>& kernel_thread, const std::vector<Watch>& watched = {});

template <class K, class... A>
Result launch(const Config& cfg, const std::vector<Watch>& watched, K kernel, A... args) {
    return run(cfg, [=]() { kernel(args...); }, watched);
}

}  // namespace hostsim

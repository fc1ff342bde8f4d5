// toy_kernels.cpp -- small kernels with known faults, for the executor's own checks (tests/test_large_hostsim.py, item 6):
// without them a silent executor would make every test of the large kernels pass.
#include <cstring>
#include <string>

#include "host_entry.hpp"
#include <hip/hip_runtime.h>

namespace {

constexpr int kToyThreads = 256, kToyLds = 2 * kToyThreads;

// `rounds` reversals of a row of blockDim.x floats through LDS, two barriers each: out[r][u] = in[r][T-1-u]
// FAULT 0: as it should be.  1: no barrier between the write and the partner's read.  2: odd threads take one barrier more.
// 3: reads a slot nobody wrote.  4: writes one float past the image.  5: writes one float in front of the output.
// 6: the threads of the upper half return before the first barrier
template <int FAULT>
__global__ void toy_reverse(const float* in, float* out, int rounds) {
    __shared__ float lds[kToyLds];
    const int u = threadIdx.x, T = blockDim.x;
    const float* row_in = in + (long)blockIdx.x * rounds * T;
    float* row_out = out + (long)blockIdx.x * rounds * T;
    if (FAULT == 6 && u >= T / 2) return;
    for (int r = 0; r < rounds; ++r) {
        lds[u] = row_in[r * T + u];
        if (FAULT != 1) __syncthreads();
        row_out[r * T + u] = lds[FAULT == 3 ? T + u : T - 1 - u];
        __syncthreads();      // the image is free for the next round
        if (FAULT == 2 && (u & 1)) __syncthreads();
    }
    if (FAULT == 4 && u == 0) lds[2 * T] = 1.f;      // (T = 256 at run time: index kToyLds)
    if (FAULT == 5 && u == 0 && blockIdx.x == 0) out[-1] = 1.f;
}

using Toy = void (*)(const float*, float*, int);
const Toy kToys[] = {toy_reverse<0>, toy_reverse<1>, toy_reverse<2>, toy_reverse<3>, toy_reverse<4>, toy_reverse<5>, toy_reverse<6>};
std::string toy_error;

}  // namespace

extern "C" {

const char* hostsim_toy_last_error() { return toy_error.c_str(); }

// in / out: grid * rounds rows of 256 floats; guard_bytes as hostsim_large_run.  Returns hostsim::Error.
int hostsim_toy_run(int fault, const float* in, float* out, int rounds, int grid, int schedule, unsigned long long seed, int blocks_descending,
                    int knock_out, int period, long guard_bytes, long* barriers) {
    if (fault < 0 || fault > 6) return -1;
    const hostsim::Config cfg = hostsim::config(kToyThreads, sizeof(float) * kToyLds, grid, schedule, seed, blocks_descending, knock_out, period);
    std::vector<hostsim::Watch> watched;
    const size_t bytes = sizeof(float) * kToyThreads * (size_t)rounds * (size_t)grid;
    hostsim::watch(watched, guard_bytes, in, bytes);
    hostsim::watch(watched, guard_bytes, out, bytes);
    return hostsim::finish(hostsim::launch(cfg, watched, kToys[fault], in, out, rounds), barriers, toy_error);
}

}  // extern "C"

// large_host.cpp -- the eight single-pass large kernels (include/smfft/smfft_large.hpp, smfft_large_real.hpp: the headers' own
// code, compiled for the host against tests/hostsim/hip/hip_runtime.h) behind C entry points that run them through the executor.
#include <cstring>
#include <string>

#include "host_entry.hpp"
#include "smfft/smfft_large_real.hpp"

namespace {

using Launcher = hostsim::Result (*)(const hostsim::Config&, const std::vector<hostsim::Watch>&, const void*, void*, int);

template <int N, int DIR>
hostsim::Result run_c2c(const hostsim::Config& cfg, const std::vector<hostsim::Watch>& w, const void* in, void* out, int nffts) {
    return hostsim::launch(cfg, w, &smfft::large::large_c2c<N, DIR>, (const float2*)in, (float2*)out, nffts);
}
template <int N>
hostsim::Result run_r2c(const hostsim::Config& cfg, const std::vector<hostsim::Watch>& w, const void* in, void* out, int nffts) {
    return hostsim::launch(cfg, w, &smfft::large::large_r2c<N>, (const float*)in, (float2*)out, nffts);
}
template <int N>
hostsim::Result run_c2r(const hostsim::Config& cfg, const std::vector<hostsim::Watch>& w, const void* in, void* out, int nffts) {
    return hostsim::launch(cfg, w, &smfft::large::large_c2r<N>, (const float2*)in, (float*)out, nffts);
}

struct Kernel {
    const char* name;
    int threads;
    long lds_bytes, fft_bytes;      // the image; one FFT's input = output bytes
    Launcher run;
};
template <int L>
using G = smfft::large::LargeGeometry<L>;
const Kernel kKernels[] = {
    {"large_c2c<8192, 0>", G<8192>::T, G<8192>::kLdsBytes, 8192 * 8, run_c2c<8192, 0>},
    {"large_c2c<8192, 1>", G<8192>::T, G<8192>::kLdsBytes, 8192 * 8, run_c2c<8192, 1>},
    {"large_c2c<16384, 0>", G<16384>::T, G<16384>::kLdsBytes, 16384 * 8, run_c2c<16384, 0>},
    {"large_c2c<16384, 1>", G<16384>::T, G<16384>::kLdsBytes, 16384 * 8, run_c2c<16384, 1>},
    {"large_r2c<16384>", G<8192>::T, G<8192>::kLdsBytes, 16384 * 4, run_r2c<16384>},
    {"large_c2r<16384>", G<8192>::T, G<8192>::kLdsBytes, 16384 * 4, run_c2r<16384>},
    {"large_r2c<32768>", G<16384>::T, G<16384>::kLdsBytes, 32768 * 4, run_r2c<32768>},
    {"large_c2r<32768>", G<16384>::T, G<16384>::kLdsBytes, 32768 * 4, run_c2r<32768>},
};

std::string last_error;

}  // namespace

extern "C" {

const char* hostsim_last_error() { return last_error.c_str(); }
unsigned hostsim_lds_prefill() { return hostsim::kLdsPrefill; }

// Runs kernel `name` (the inventory's name without "smfft::large::") on nFFTs FFTs with a host grid of `grid` workgroups.
// schedule / seed / blocks_descending: hostsim::Config.  knock_out >= 0 with period P: barrier knock_out of every P is absent.
// guard_bytes > 0: the caller keeps that many bytes on either side of both buffers, which must not change.
// barriers[grid] (may be null) receives each workgroup's barrier count.  Returns hostsim::Error, -1 for an unknown kernel.
int hostsim_large_run(const char* name, const void* d_input, void* d_output, int nFFTs, int grid, int schedule, unsigned long long seed,
                      int blocks_descending, int knock_out, int period, long guard_bytes, long* barriers) {
    for (const Kernel& k : kKernels) {
        if (std::strcmp(k.name, name) != 0) continue;
        const hostsim::Config cfg = hostsim::config(k.threads, (size_t)k.lds_bytes, grid, schedule, seed, blocks_descending, knock_out, period);
        std::vector<hostsim::Watch> watched;
        const size_t bytes = (size_t)k.fft_bytes * (size_t)(nFFTs > 0 ? nFFTs : 0);
        hostsim::watch(watched, guard_bytes, d_input, bytes);
        if (d_output != d_input) hostsim::watch(watched, guard_bytes, d_output, bytes);
        return hostsim::finish(k.run(cfg, watched, d_input, d_output, nFFTs), barriers, last_error);
    }
    last_error = std::string("unknown kernel ") + name;
    return -1;
}

}  // extern "C"

// large_fir_host.cpp -- the overlap-save filter-bank kernels of include/smfft/smfft_large_fir.hpp (the header's own code, compiled for
// the host against tests/hostsim/hip/hip_runtime.h) behind C entry points that run them through the executor.  Both forms of the
// filter loop are here, whichever the library ships.
#include <cstring>
#include <string>

#include "host_entry.hpp"
#include "smfft/smfft_large_fir.hpp"

namespace {

using smfft::FirWindow;
using FirLauncher = hostsim::Result (*)(const hostsim::Config&, const std::vector<hostsim::Watch>&, const float2*, const float2*, float2*, FirWindow, int, int, long long);      // x, H, y, w, K, group, units
using PrepareLauncher = hostsim::Result (*)(const hostsim::Config&, const std::vector<hostsim::Watch>&, const float2*, int, int, int, float2*);

template <int N, int HELD>
hostsim::Result run_fir(const hostsim::Config& cfg, const std::vector<hostsim::Watch>& watched, const float2* x, const float2* H, float2* y, FirWindow w,
                        int K, int group, long long units) {
    const smfft::large::LargeFirStride st = smfft::large::large_fir_stride(cfg.grid, (K + group - 1) / group, w.segments());
    return hostsim::launch(cfg, watched, &smfft::large::large_fir<N, HELD>, x, H, y, w, K, group, units, st);
}
template <int N>
hostsim::Result run_prepare(const hostsim::Config& cfg, const std::vector<hostsim::Watch>& watched, const float2* taps, int M, int K, int correlate,
                            float2* spectra) {
    return hostsim::launch(cfg, watched, &smfft::large::large_fir_prepare<N>, taps, M, K, correlate, spectra);
}

struct Kernel {
    const char* name;
    int N, held;
    FirLauncher fir;
    PrepareLauncher prepare;
};
const Kernel kKernels[] = {
    {"large_fir<8192, 0>", 8192, 0, run_fir<8192, 0>, nullptr},
    {"large_fir<8192, 1>", 8192, 1, run_fir<8192, 1>, nullptr},
    {"large_fir<16384, 0>", 16384, 0, run_fir<16384, 0>, nullptr},
    {"large_fir_prepare<8192>", 8192, 0, nullptr, run_prepare<8192>},
    {"large_fir_prepare<16384>", 16384, 0, nullptr, run_prepare<16384>},
};

std::string last_error;

const Kernel* find(const char* name) {
    for (const Kernel& k : kKernels)
        if (std::strcmp(k.name, name) == 0) return &k;
    last_error = std::string("unknown kernel ") + name;
    return nullptr;
}

hostsim::Config config(int N, int grid, int schedule, unsigned long long seed, int blocks_descending, int knock_out, int period) {
    const size_t lds = N == 8192 ? smfft::large::LargeGeometry<8192>::kLdsBytes : smfft::large::LargeGeometry<16384>::kLdsBytes;
    return hostsim::config(N / 16, lds, grid, schedule, seed, blocks_descending, knock_out, period);
}

}  // namespace

extern "C" {

const char* hostsim_large_fir_last_error() { return last_error.c_str(); }
unsigned hostsim_large_fir_lds_prefill() { return hostsim::kLdsPrefill; }

// Runs filter kernel `name` over C channels of L samples and K prepared spectra on a host grid of `grid` workgroups.  group_size:
// filters per unit of the held form (the recompute form takes 1).  schedule / seed / blocks_descending / knock_out / period:
// hostsim::Config.  guard_bytes > 0: the caller keeps that many bytes on either side of the three buffers, which must not change.
// barriers[grid] (may be null) receives each workgroup's barrier count; *units the number of units of the launch.
// Returns hostsim::Error, -1 for an unknown kernel or an argument the launcher of the library would refuse.
int hostsim_large_fir_run(const char* name, const void* x, const void* H, void* y, long long L, int C, int K, int M, int correlate, int group_size,
                          int grid, int schedule, unsigned long long seed, int blocks_descending, int knock_out, int period, long guard_bytes,
                          long* barriers, long long* units_out) {
    const Kernel* k = find(name);
    if (!k || !k->fir) return -1;
    if (L < 1 || C < 1 || K < 1 || M < 1 || M >= k->N || group_size < 1 || (!k->held && group_size != 1)) {
        last_error = "bad filter-bank arguments";
        return -1;
    }
    const FirWindow w{L, k->N, M, correlate != 0};
    const long long units = w.segments() * C * ((K + group_size - 1) / group_size);
    if (units_out) *units_out = units;
    std::vector<hostsim::Watch> watched;
    hostsim::watch(watched, guard_bytes, x, (size_t)C * L * 8);
    hostsim::watch(watched, guard_bytes, H, (size_t)K * k->N * 8);
    hostsim::watch(watched, guard_bytes, y, (size_t)C * K * L * 8);
    const hostsim::Config cfg = config(k->N, grid, schedule, seed, blocks_descending, knock_out, period);
    return hostsim::finish(k->fir(cfg, watched, (const float2*)x, (const float2*)H, (float2*)y, w, K, group_size, units), barriers, last_error);
}

// Runs the prepare kernel `name` on K filters of M taps.
int hostsim_large_fir_prepare(const char* name, const void* taps, int M, int K, int correlate, void* spectra, int grid, int schedule,
                              unsigned long long seed, long guard_bytes, long* barriers) {
    const Kernel* k = find(name);
    if (!k || !k->prepare) return -1;
    if (K < 1 || M < 1 || M >= k->N) {
        last_error = "bad prepare arguments";
        return -1;
    }
    std::vector<hostsim::Watch> watched;
    hostsim::watch(watched, guard_bytes, taps, (size_t)K * M * 8);
    hostsim::watch(watched, guard_bytes, spectra, (size_t)K * k->N * 8);
    const hostsim::Config cfg = config(k->N, grid, schedule, seed, 0, -1, 0);
    return hostsim::finish(k->prepare(cfg, watched, (const float2*)taps, M, K, correlate, (float2*)spectra), barriers, last_error);
}

}  // extern "C"

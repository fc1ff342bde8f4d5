// large_pfb_host.cpp -- the polyphase filter bank kernels of include/smfft/smfft_large_pfb.hpp (the header's own code, compiled for the
// host against tests/hostsim/hip/hip_runtime.h) behind a C entry point that runs them through the executor.
#include <string>

#include "host_entry.hpp"
#include "smfft/smfft_large_pfb.hpp"

namespace {

using smfft::PfbPlan;
using smfft::large::LargePfbSchedule;
using Launcher = hostsim::Result (*)(const hostsim::Config&, const std::vector<hostsim::Watch>&, const float2*, const float*, void*, PfbPlan, LargePfbSchedule);

template <int N, int POWER>
hostsim::Result run_pfb(const hostsim::Config& cfg, const std::vector<hostsim::Watch>& watched, const float2* x, const float* h, void* y, PfbPlan plan,
                        LargePfbSchedule sched) {
    return hostsim::launch(cfg, watched, &smfft::large::pfb_large<N, POWER, 0>, x, h, y, plan, sched);
}

std::string last_error;

}  // namespace

extern "C" {

const char* hostsim_large_pfb_last_error() { return last_error.c_str(); }

// Runs pfb_large<N, power> over C streams of L samples and a prototype of P N taps on a host grid of at most max_workgroups workgroups
// under the kernel's schedule `form` (1 stride, 2 XCD-blocked): the grid and the form are LargePfbSchedule::make's, as in the library's
// launcher, and are returned in grid_out[0], grid_out[1].  schedule / seed / blocks_descending / knock_out / period: hostsim::Config.
// guard_bytes > 0: the caller keeps that many bytes on either side of the three buffers, which must not change.  barriers[grid] (may
// be null) receives each workgroup's barrier count.  Returns hostsim::Error, -1 for arguments the library would refuse or a launch
// with nothing to do.
int hostsim_large_pfb_run(int N, int power, const void* x, const void* h, void* y, long long L, int C, int P, int form, int max_workgroups, int schedule,
                          unsigned long long seed, int blocks_descending, int knock_out, int period, long guard_bytes, long* barriers, int* grid_out) {
    if ((N != 8192 && N != 16384) || P < 1 || P > 32 || C < 1 || L < 0 || (form != 1 && form != 2) || max_workgroups < 1) {
        last_error = "bad filter-bank arguments";
        return -1;
    }
    const PfbPlan plan{L, N, P, C};
    if (plan.pairs() == 0) {
        last_error = "no whole frame";
        return -1;
    }
    const LargePfbSchedule sched = LargePfbSchedule::make(plan.pairs(), max_workgroups, form);
    if (grid_out) {
        grid_out[0] = sched.grid;
        grid_out[1] = sched.form;
    }
    std::vector<hostsim::Watch> watched;
    hostsim::watch(watched, guard_bytes, x, (size_t)C * L * 8);
    hostsim::watch(watched, guard_bytes, h, (size_t)P * N * 4);
    hostsim::watch(watched, guard_bytes, y, (size_t)plan.pairs() * N * (power ? 4 : 8));
    const size_t lds = N == 8192 ? smfft::large::LargeGeometry<8192>::kLdsBytes : smfft::large::LargeGeometry<16384>::kLdsBytes;
    const hostsim::Config cfg = hostsim::config(N / 16, lds, sched.grid, schedule, seed, blocks_descending, knock_out, period);
    const Launcher launcher = N == 8192 ? (power ? run_pfb<8192, 1> : run_pfb<8192, 0>) : (power ? run_pfb<16384, 1> : run_pfb<16384, 0>);
    return hostsim::finish(launcher(cfg, watched, (const float2*)x, (const float*)h, y, plan, sched), barriers, last_error);
}

}  // extern "C"

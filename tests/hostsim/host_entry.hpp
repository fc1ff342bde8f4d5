// host_entry.hpp -- what the C entry points of large_host.cpp, large_fir_host.cpp, large_pfb_host.cpp and toy_kernels.cpp share: the
// Config of a launch from the entry points' common arguments, the Watch of a guarded buffer, and the hand-back of a Result.
#pragma once
#include <string>
#include <vector>

#include "hostsim.hpp"

namespace hostsim {

inline Config config(int threads, size_t lds_bytes, int grid, int schedule, unsigned long long seed, int blocks_descending, int knock_out, int period) {
    Config cfg;
    cfg.grid = grid;
    cfg.threads = threads;
    cfg.schedule = schedule;
    cfg.seed = seed;
    cfg.blocks_descending = blocks_descending != 0;
    cfg.knock_out = knock_out;
    cfg.period = period;
    cfg.lds_bytes = lds_bytes;
    return cfg;
}

// guard_bytes > 0: the caller keeps that many bytes on either side of the buffer, which must not change
inline void watch(std::vector<Watch>& watched, long guard_bytes, const void* base, size_t bytes) {
    if (guard_bytes > 0) watched.push_back({base, bytes, (size_t)guard_bytes});
}

// the message to the entry file's last_error, each workgroup's barrier count to barriers[grid] (may be null); returns hostsim::Error
inline int finish(const Result& r, long* barriers, std::string& last_error) {
    last_error = r.message;
    if (barriers)
        for (size_t i = 0; i < r.barriers.size(); ++i) barriers[i] = r.barriers[i];
    return r.error;
}

}  // namespace hostsim

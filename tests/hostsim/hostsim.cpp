// hostsim.cpp -- the executor of hostsim.hpp.  Link this object LAST: its guard array must close the LDS section.
#include <sys/mman.h>
#include <ucontext.h>

#include <algorithm>
#include <numeric>

#include "hostsim.hpp"
#include <hip/hip_runtime.h>

// the bounds of the section that holds every __shared__ array of the program (defined by the linker)
extern "C" char __start_hostsim_lds[] __attribute__((weak));
extern "C" char __stop_hostsim_lds[] __attribute__((weak));

namespace hostsim {

uint3 thread_idx, block_idx;
dim3 block_dim, grid_dim;

// closes the section: a write past the end of the last image lands here and is seen
static __attribute__((section("hostsim_lds"), aligned(HOSTSIM_LDS_ALIGN), used)) uint32_t lds_tail_guard[16384];

void unmodelled(const char* what, const char* where) {
    std::fprintf(stderr, "hostsim: %s reached in %s: not modelled by the host executor\n", what, where);
    std::abort();
}

void asm_statement(const char* text, const char* where) {
    // the stringified statement starts with its instruction string: "" is an optimisation barrier, inert on the host
    if (text[0] == '"' && text[1] == '"') return;
    std::fprintf(stderr, "hostsim: asm statement reached in %s: %.200s\n", where, text);
    std::abort();
}

namespace {

constexpr size_t kStackBytes = 256 << 10;

struct Fiber {
    ucontext_t ctx;
    bool done = false;
    long barriers = 0;
};

struct Running {
    const Config* cfg = nullptr;
    const std::function<void()>* kernel = nullptr;
    ucontext_t scheduler;
    Fiber* current = nullptr;
} g;

void fiber_entry() {
    (*g.kernel)();
    g.current->done = true;
    swapcontext(&g.current->ctx, &g.scheduler);
}

struct Rng {      // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    void shuffle(std::vector<int>& v) {
        for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[next() % i]);
    }
};

void interval_order(const Config& cfg, Rng& rng, std::vector<int>& order) {
    const int T = cfg.threads;
    order.resize(T);
    std::iota(order.begin(), order.end(), 0);
    if (cfg.schedule == kDescending) {
        std::reverse(order.begin(), order.end());
    } else if (cfg.schedule == kWaves) {
        std::vector<int> waves((T + 63) / 64);
        std::iota(waves.begin(), waves.end(), 0);
        rng.shuffle(waves);
        order.clear();
        for (int w : waves)
            for (int t = 64 * w; t < std::min(T, 64 * w + 64); ++t) order.push_back(t);
    } else if (cfg.schedule == kRandom) {
        rng.shuffle(order);
    }
}

void lds_fill() {
    uint32_t* p = (uint32_t*)__start_hostsim_lds;
    std::fill(p, (uint32_t*)__stop_hostsim_lds, kLdsPrefill);
}

// every changed word must lie in the image that starts at the 1 MiB boundary below the first changed one
bool lds_check(const Config& cfg, std::string& why) {
    const uint32_t* p = (const uint32_t*)__start_hostsim_lds;
    const size_t words = (__stop_hostsim_lds - __start_hostsim_lds) / 4;
    size_t first = words, last = 0;
    for (size_t i = 0; i < words; ++i)
        if (p[i] != kLdsPrefill) {
            if (first == words) first = i;
            last = i;
        }
    if (first == words) return true;
    const size_t base = first * 4 / HOSTSIM_LDS_ALIGN * HOSTSIM_LDS_ALIGN;
    if (last * 4 + 4 - base <= cfg.lds_bytes) return true;
    why = "LDS write outside the image: byte " + std::to_string(last * 4 - base) + " of an image of " + std::to_string(cfg.lds_bytes);
    return false;
}

}  // namespace

void barrier() {
    Fiber* f = g.current;
    const long i = f->barriers++;
    if (g.cfg->period > 0 && g.cfg->knock_out >= 0 && i % g.cfg->period == g.cfg->knock_out) return;
    swapcontext(&f->ctx, &g.scheduler);
}

Result run(const Config& cfg, const std::function<void()>& kernel_thread, const std::vector<Watch>& watched) {
    Result res;
    auto fail = [&](int e, const std::string& m) -> Result& {
        res.error = e;
        res.message = m;
        return res;
    };
    if (cfg.grid < 0 || cfg.threads < 1 || cfg.schedule < kAscending || cfg.schedule > kRandom || (cfg.knock_out >= 0 && cfg.knock_out >= cfg.period))
        return fail(kBadLaunch, "bad launch configuration");
    if (g.cfg) return fail(kBadLaunch, "a launch is running: the executor is not re-entrant");
    if (!__start_hostsim_lds || (char*)(lds_tail_guard + 16384) != __stop_hostsim_lds)
        return fail(kBadLaunch, "hostsim.cpp must be the last object of the link (its guard closes the LDS section)");

    std::vector<std::vector<unsigned char>> guards;
    for (const Watch& w : watched) {
        const unsigned char* b = (const unsigned char*)w.base;
        guards.emplace_back(b - w.guard, b);
        guards.emplace_back(b + w.bytes, b + w.bytes + w.guard);
    }

    const int T = cfg.threads;
    char* stacks = (char*)mmap(nullptr, kStackBytes * T, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (stacks == MAP_FAILED) return fail(kBadLaunch, "no memory for the fibers' stacks");
    std::vector<Fiber> fibers(T);
    std::vector<int> order;
    Rng rng{cfg.seed * 0x2545f4914f6cdd1dull + (uint64_t)cfg.schedule};
    g.cfg = &cfg;
    g.kernel = &kernel_thread;
    block_dim = dim3(T);
    grid_dim = dim3(cfg.grid);
    res.barriers.assign(cfg.grid, 0);

    for (int n = 0; n < cfg.grid && res.error == kOk; ++n) {
        const int wg = cfg.blocks_descending ? cfg.grid - 1 - n : n;
        lds_fill();
        for (int t = 0; t < T; ++t) {
            Fiber& f = fibers[t];
            f.done = false;
            f.barriers = 0;
            getcontext(&f.ctx);
            f.ctx.uc_stack.ss_sp = stacks + kStackBytes * t;
            f.ctx.uc_stack.ss_size = kStackBytes;
            f.ctx.uc_link = nullptr;
            makecontext(&f.ctx, fiber_entry, 0);
        }
        for (;;) {
            interval_order(cfg, rng, order);
            int done = 0;
            for (int t : order) {
                Fiber& f = fibers[t];
                if (f.done) continue;       // (only after a divergence, which ends the launch below)
                g.current = &f;
                thread_idx = uint3{(unsigned)t, 0, 0};
                block_idx = uint3{(unsigned)wg, 0, 0};
                swapcontext(&g.scheduler, &f.ctx);
                done += f.done;
            }
            if (done == T) break;
            if (done != 0) {
                fail(kDivergentBarrier, "workgroup " + std::to_string(wg) + ": " + std::to_string(done) + " of " + std::to_string(T) +
                                            " threads ended while the others wait at a barrier");
                break;
            }
        }
        if (res.error != kOk) break;
        res.barriers[wg] = fibers[0].barriers;
        for (int t = 1; t < T; ++t)
            if (fibers[t].barriers != fibers[0].barriers) {
                fail(kDivergentBarrier, "workgroup " + std::to_string(wg) + ": thread " + std::to_string(t) + " reached " +
                                            std::to_string(fibers[t].barriers) + " barriers, thread 0 " + std::to_string(fibers[0].barriers));
                break;
            }
        std::string why;
        if (res.error == kOk && !lds_check(cfg, why)) fail(kLdsOutOfBounds, "workgroup " + std::to_string(wg) + ": " + why);
    }
    g.cfg = nullptr;
    g.kernel = nullptr;
    g.current = nullptr;
    munmap(stacks, kStackBytes * T);

    if (res.error == kOk) {
        size_t i = 0;
        for (const Watch& w : watched) {
            const unsigned char* b = (const unsigned char*)w.base;
            if (!std::equal(guards[i].begin(), guards[i].end(), b - w.guard) || !std::equal(guards[i + 1].begin(), guards[i + 1].end(), b + w.bytes)) {
                fail(kGlobalOutOfBounds, "watched buffer " + std::to_string(i / 2) + ": a guard band was written");
                break;
            }
            i += 2;
        }
    }
    return res;
}

}  // namespace hostsim

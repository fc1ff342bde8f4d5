// smfft_api.hip -- host side of libsmfft_amd.so: the C ABI of include/smfft.h and the reference's
// own C++-linkage entry points (include/smfft_reference_api.h).
//
// Mirrors, in behaviour (return codes, printed lines, timing convention), the host code of the
// three reference programs: CT:576-752 + :827-908, ST:299-384 + :457-530, RC:388-467 + :572-688.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <climits>
#include <map>
#include <mutex>
#include <utility>

#include "../../include/smfft.h"
#include "../../include/smfft_debug.h"
#include "../../include/smfft_reference_api.h"
#include "smfft_host_util.hpp"
#include "smfft_launch.hpp"
#include "smfft_pairs.hpp"
#include "smfft_state.hpp"

namespace {

// Launch state.  Upstream has process globals (`int device = 0`, CT:15) and one host thread.  Here every host thread has
// its own device / grid cap / applications-per-slot / pacing, so that N threads can drive N GPUs through the unchanged
// prototypes (GPU_smFFT_4elements and friends included); a value a thread has not set falls back to the process default
// (environment: SMFFT_DEVICE, SMFFT_GRID_CAP, SMFFT_PACING, read once).  The lanes of smfft_host_transform inherit the
// state of the thread that called it (smfft_state.hpp).
smfft::LaunchState g_defaults = {0, 12288, SMFFT_NREUSES, -1, 1, 15, 1000, -1, 0, 0};   // 12288 workgroups per launch: grid-stride over tiles, 12 or 16
                                                                 // rounds of the 4 or 3 resident workgroups per CU (measured sweet spot)
thread_local smfft::LaunchState t_state = {-1, smfft::kUnsetGridCap, 0, -2, -1, -1, -1, -1, 0, 0};
std::once_flag g_env_once;

// launches may come from several host threads (per-GPU threads of a multi-GPU driver, the lanes of
// smfft_host_transform): the environment is read exactly once
void read_env() {
    std::call_once(g_env_once, [] {
        if (const char* e = getenv("SMFFT_GRID_CAP")) g_defaults.grid_cap = atoi(e);
        if (const char* e = getenv("SMFFT_DEVICE")) g_defaults.device = atoi(e);
        if (const char* e = getenv("SMFFT_PACING")) g_defaults.pacing = atoi(e) > 0 ? atoi(e) : 0;
        if (const char* e = getenv("SMFFT_MULT_BALANCE")) g_defaults.balance = atoi(e) > 0 ? atoi(e) : 0;
        if (const char* e = getenv("SMFFT_PRIO_ROTATE")) g_defaults.rotate = atoi(e) > 0 ? atoi(e) : 0;
        if (const char* e = getenv("SMFFT_HANDOFF_WAIT_US")) g_defaults.handoff_wait_us = atoi(e) > 0 ? atoi(e) : 0;
    });
}
int cur_device() { return t_state.device >= 0 ? t_state.device : g_defaults.device; }
int cur_grid_cap() { return t_state.grid_cap != smfft::kUnsetGridCap ? t_state.grid_cap : g_defaults.grid_cap; }
int cur_nreuses() { return t_state.nreuses > 0 ? t_state.nreuses : g_defaults.nreuses; }
int cur_rotate() { return t_state.rotate >= 0 ? t_state.rotate : g_defaults.rotate; }
int cur_balance() { return t_state.balance >= 0 ? t_state.balance : g_defaults.balance; }
int cur_pacing() { return t_state.pacing != -2 ? t_state.pacing : g_defaults.pacing; }   // -1: chosen per launch from the output buffer
smfft::LaunchOptions cur_options(int pace) {
    smfft::LaunchOptions o = {};
    o.grid_cap = cur_grid_cap();
    o.nreuses = cur_nreuses();
    o.pace = pace;
    o.balance = cur_balance();
    o.rotate = cur_rotate();
    o.handoff_wait_us = (unsigned)(t_state.handoff_wait_us >= 0 ? t_state.handoff_wait_us : g_defaults.handoff_wait_us);
    o.delay_chain = t_state.delay_chain;
    o.delay_ms = (unsigned)t_state.delay_ms;
    o.delay_after_commit = t_state.delay_after_commit;
    return o;
}

// count of FFT slots the `multiple` path touches (CT:669-683; ST:351; RC:438)
int ct_multiple_slots(int FFT_size, int nFFTs) {
    if (FFT_size == 32) return (nFFTs / (4 * SMFFT_NREUSES)) * 4;
    if (FFT_size == 64) return (nFFTs / (2 * SMFFT_NREUSES)) * 2;
    return nFFTs / SMFFT_NREUSES;
}

// K > 0: the external kernels run their rate limiter with K loads for this output buffer: k_ordinary when it is ordinary
// memory, k_mixed when it is one of the mixed outputs smfft_malloc_pair built (smfft_pairs.hip)
int pacing_for(const void* d_output, int k_ordinary, int k_mixed);
// serialised LDS loads between a wave's loads and stores, by transform length (sweeps on the same buffers:
// tools/pacing_sweep.py, profiles/r02_pacing_sweep_plain.txt / _pair.txt)
struct Pacing { int ordinary, mixed; };
Pacing c2c_pacing(int N) { return {N <= 1024 ? 12 : 8, N <= 2048 ? 4 : 0}; }
Pacing rc_pacing(int L) { return {L == 512 ? 6 : L == 1024 ? 8 : 0, 0}; }

using smfft::launch_ct;
using smfft::launch_rc;
using smfft::launch_st;

// returns -1 for an unsupported length (nothing launched), else the launch status
int dispatch_ct(const float2* in, float2* out, int N, int count, int inverse, int reorder, int path, hipStream_t st) {
    const smfft::LaunchOptions opt = cur_options(pacing_for(out, c2c_pacing(N).ordinary, c2c_pacing(N).mixed));
    switch (N) {
        case 32:   return launch_ct<32>(in, out, count, inverse, reorder, path, opt, st);
        case 64:   return launch_ct<64>(in, out, count, inverse, reorder, path, opt, st);
        case 128:  return launch_ct<128>(in, out, count, inverse, reorder, path, opt, st);
        case 256:  return launch_ct<256>(in, out, count, inverse, reorder, path, opt, st);
        case 512:  return launch_ct<512>(in, out, count, inverse, reorder, path, opt, st);
        case 1024: return launch_ct<1024>(in, out, count, inverse, reorder, path, opt, st);
        case 2048: return launch_ct<2048>(in, out, count, inverse, reorder, path, opt, st);
        case 4096: return launch_ct<4096>(in, out, count, inverse, reorder, path, opt, st);
        default:   return -1;
    }
}
int dispatch_st(const float2* in, float2* out, int N, int count, int path, hipStream_t st) {
    const smfft::LaunchOptions opt = cur_options(pacing_for(out, c2c_pacing(N).ordinary, c2c_pacing(N).mixed));
    switch (N) {
        case 32:   return launch_st<32>(in, out, count, path, opt, st);
        case 64:   return launch_st<64>(in, out, count, path, opt, st);
        case 128:  return launch_st<128>(in, out, count, path, opt, st);
        case 256:  return launch_st<256>(in, out, count, path, opt, st);
        case 512:  return launch_st<512>(in, out, count, path, opt, st);
        case 1024: return launch_st<1024>(in, out, count, path, opt, st);
        case 2048: return launch_st<2048>(in, out, count, path, opt, st);
        case 4096: return launch_st<4096>(in, out, count, path, opt, st);
        default:   return -1;
    }
}
// the DIF transform (natural order in, bit-reversed spectrum out): its own entry points, no reorder / family value of its own
int dispatch_dif(const float2* in, float2* out, int N, int count, int inverse, hipStream_t st) {
    switch (N) {
        case 32:   return smfft::launch_dif<32>(in, out, count, inverse, st);
        case 64:   return smfft::launch_dif<64>(in, out, count, inverse, st);
        case 128:  return smfft::launch_dif<128>(in, out, count, inverse, st);
        case 256:  return smfft::launch_dif<256>(in, out, count, inverse, st);
        case 512:  return smfft::launch_dif<512>(in, out, count, inverse, st);
        case 1024: return smfft::launch_dif<1024>(in, out, count, inverse, st);
        case 2048: return smfft::launch_dif<2048>(in, out, count, inverse, st);
        case 4096: return smfft::launch_dif<4096>(in, out, count, inverse, st);
        default:   return -1;
    }
}
// FFT_size is the REAL length; the kernels are instantiated on the complex length L = FFT_size/2 (RC:404-428)
int dispatch_rc(const float2* in, float2* out, int FFT_size, int count, int inverse, int path, hipStream_t st) {
    const smfft::LaunchOptions opt = cur_options(pacing_for(out, rc_pacing(FFT_size / 2).ordinary, rc_pacing(FFT_size / 2).mixed));
    switch (FFT_size) {
        case 512:  return launch_rc<256>(in, out, count, inverse, path, opt, st);
        case 1024: return launch_rc<512>(in, out, count, inverse, path, opt, st);
        case 2048: return launch_rc<1024>(in, out, count, inverse, path, opt, st);
        case 4096: return launch_rc<2048>(in, out, count, inverse, path, opt, st);
        default:   return -1;
    }
}

// One event-timed launch on stream 0, elapsed ms ADDED to *FFT_time (CT:598,660-662).
template <class F>
int timed(F&& launch, double* FFT_time) {
    read_env();
    GpuTimer timer;
    timer.Start();
    int rc = launch();
    timer.Stop();
    if (rc == -1) printf("Error wrong FFT length!\n");
    else if (rc != 0) checkHipErrors((hipError_t)rc);
    if (FFT_time) *FFT_time += timer.Elapsed();
    return 0;
}

// The paired-buffer allocator (smfft_malloc_pair and friends; what the L3 wrappers take their buffers from) is a translation
// unit of its own: smfft_pairs.hip / smfft_pairs.hpp.
using smfft::pairs::alloc_pair;
using smfft::pairs::alloc_pair_for_wrapper;
using smfft::pairs::free_pair;
int pacing_for(const void* d_output, int k_ordinary, int k_mixed) { return smfft::pairs::pacing_for(d_output, k_ordinary, k_mixed, cur_pacing()); }

// The wrappers' memory test (CT:844-847: "2 * bytes > free_mem").  What the device must hold is the pair; what the wrapper MAY
// hold while it allocates is more -- the placement search scans chunks on top of the pair, bounded by its byte budget and by what
// is free after the pair less 1 GiB (smfft_pairs.hpp, wrapper_peak_bytes), and it shrinks to fit, so it never turns a request
// that fits into one that fails.  A pair the previous wrapper call left in the cache is either re-used (same size: nothing is
// allocated, the test is skipped) or released before the new pair is allocated, so its bytes count as available.
// false: "not enough memory" (the caller prints the reference's line and returns 1).
bool wrapper_memory_ok(size_t pair_bytes_each, size_t needed, size_t free_mem) {
    int device = 0;
    (void)hipGetDevice(&device);
    if (smfft::pairs::cache_would_serve(pair_bytes_each, device)) return true;
    const size_t available = free_mem + smfft::pairs::cached_bytes(device);
    if (DEBUG) printf("  The device buffers need %0.3f MB; while they are allocated the placement search may hold up to %0.3f MB.\n", (float)needed / (1024.0 * 1024.0),
                      (float)smfft::pairs::wrapper_peak_bytes(pair_bytes_each, available) / (1024.0 * 1024.0));
    return needed <= available;
}


// The L3 wrappers time nRuns launches right after a multi-GiB upload, i.e. on a device whose shader clock has fallen back: the
// first tens of milliseconds of in-LDS launches then run 20-40 % under the settled rate (clocks follow the load on MI355X;
// profiles/r03_warm_ramp.txt), and with upstream's nRuns = 20 the reported mean is mostly ramp.  The wrappers therefore run the
// SAME launch untimed until it has accumulated SMFFT_WRAPPER_WARMUP_MS of kernel time, then time nRuns launches exactly as upstream
// does (CT:862-871).  DEFAULT 0 (round 6): upstream times its nRuns launches directly behind the upload, and so does the wrapper
// unless the variable asks otherwise (tools/readme_table.py sets 40 for the settled figures and says so; bench.py does not go
// through the wrappers).  The results are the same launches' results.
template <class F>
void wrapper_warm_up(F&& timed_launch) {
    static const double budget = [] { const char* e = getenv("SMFFT_WRAPPER_WARMUP_MS"); return e ? atof(e) : 0.0; }();
    double spent = 0;
    for (int i = 0; i < 4096 && spent < budget; ++i) {
        const double before = spent;
        timed_launch(&spent);
        if (!(spent > before)) break;            // nothing ran (unsupported length, batch too small): nothing to warm up
    }
}

int select_device() {
    read_env();
    int devCount = 0;
    checkHipErrors(hipGetDeviceCount(&devCount));
    if (devCount > cur_device()) checkHipErrors(hipSetDevice(cur_device()));
    return devCount;
}

}  // namespace

namespace smfft {
LaunchState get_thread_state() { return t_state; }
void set_thread_state(const LaunchState& s) { t_state = s; }

// ---- host side of the multiple paths' balanced schedule (smfft_kernels.hpp, MultipleSchedule) -----------------------------
// Workgroups of `kernel` that the device holds at once, from the kernel's own resources and the CU's: the vector registers of a
// SIMD lane (handed out to a wave in blocks), the wave slots of a SIMD, the LDS of a CU.  The register file is not a device
// attribute, so it is a table by architecture (MI355X_MICROARCH.md: gfx950 -- 512 registers per lane in blocks of 8, 8 wave slots
// per SIMD); the LDS comes from the device.  On an architecture the table does not know the answer is 0 and the multiple paths run
// one chain per workgroup (nothing is assumed about a device nobody has counted on).  hipOccupancyMaxActiveBlocksPerMultiprocessor
// counts the LDS only -- it answered 19 per CU for a 126-register single-wave kernel of which 16 run (profiles/r04_workgroup_trace.txt)
// -- so it serves as an upper bound here; tests/test_gpu_parity.py checks this function against smfft_measure_multiple_residency,
// which COUNTS the workgroups that are alive at once, for every kernel.  (numRegs counts the arch VGPRs; none of the kernels uses AGPRs.)
struct RegisterFile { const char* arch; int per_lane, granule, wave_slots; };
static const RegisterFile kRegisterFiles[] = {{"gfx950", 512, 8, 8}, {"gfx942", 512, 8, 8}, {"gfx90a", 512, 8, 8}};
int resident_workgroups(const void* kernel, int threads) {
    static std::mutex mutex;
    static std::map<std::pair<const void*, int>, int> known;      // (kernel, device) -> workgroups
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) { (void)hipGetLastError(); return 0; }
    std::lock_guard<std::mutex> lock(mutex);
    auto it = known.find({kernel, device});
    if (it != known.end()) return it->second;
    int result = 0;
    hipFuncAttributes attr = {};
    hipDeviceProp_t prop = {};
    const RegisterFile* rf = nullptr;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess)
        for (const RegisterFile& r : kRegisterFiles)
            if (strncmp(prop.gcnArchName, r.arch, strlen(r.arch)) == 0) rf = &r;
    int lds_per_cu = 0, by_runtime = 0;
    if (rf && hipFuncGetAttributes(&attr, kernel) == hipSuccess && attr.numRegs > 0 && prop.multiProcessorCount > 0 &&
        hipDeviceGetAttribute(&lds_per_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, device) == hipSuccess && lds_per_cu > 0) {
        const int regs = (attr.numRegs + rf->granule - 1) / rf->granule * rf->granule;
        int waves_per_simd = rf->per_lane / regs;
        if (waves_per_simd > rf->wave_slots) waves_per_simd = rf->wave_slots;
        const int waves_per_wg = (threads + 63) / 64;
        int per_cu = waves_per_simd * 4 / waves_per_wg;
        if (attr.sharedSizeBytes > 0) {
            const int by_lds = (int)((size_t)lds_per_cu / attr.sharedSizeBytes);
            if (by_lds < per_cu) per_cu = by_lds;
        }
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&by_runtime, kernel, threads, 0) == hipSuccess && by_runtime > 0 && by_runtime < per_cu) per_cu = by_runtime;
        if (per_cu > 32) per_cu = 32;
        result = per_cu * prop.multiProcessorCount;
    }
    (void)hipGetLastError();
    return known[{kernel, device}] = result;
}
thread_local unsigned* t_residency_probe = nullptr;
thread_local int t_last_slots = 0;
void note_resident_workgroups(int slots) { t_last_slots = slots; }
int last_noted_slots() { return t_last_slots; }
unsigned* residency_probe() { return t_residency_probe; }

// The hand-over words of the balanced launches: a pool of fixed-size buffers per device.  A launch takes one that no launch in
// flight uses (its event has completed, or it has never been used), and gives it back by recording an event behind the kernel:
// launches that can overlap -- other streams, hipStreamPerThread of other host threads, other host threads on the same stream --
// never share words, nothing is keyed by a stream handle (which a destroyed stream's successor may reuse), and nothing in the
// launch path frees memory.  The pool is bounded; when every buffer is in flight the launch runs unbalanced.
struct ScheduleBuffer {
    int device = -1;
    unsigned* flags = nullptr;
    unsigned epoch = 0;
    hipEvent_t done = nullptr;
    bool in_flight = false;      // an event has been recorded behind the last launch that used it
    bool taken = false;          // between schedule_acquire and schedule_release
};
constexpr int kSchedulePool = 32;
static std::mutex g_schedule_mutex;
static ScheduleBuffer g_schedule_pool[kSchedulePool];
unsigned* schedule_acquire(int nchains, hipStream_t stream, unsigned* base, int* ticket) {
    *ticket = -1;
    if (nchains > kScheduleMaxChains) return nullptr;
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    std::lock_guard<std::mutex> lock(g_schedule_mutex);
    int chosen = -1, empty = -1;
    for (int i = 0; i < kSchedulePool && chosen < 0; ++i) {
        ScheduleBuffer& b = g_schedule_pool[i];
        if (!b.flags) { if (empty < 0) empty = i; continue; }
        if (b.device != device || b.taken) continue;
        if (b.in_flight) {
            // Recycled on hipSuccess ONLY.  Any other answer -- not ready, or an error of the query itself (a context error; another
            // thread's global-mode stream capture makes the call illegal) -- says nothing about the launch that used the buffer, and two
            // launches sharing hand-over words under different bases would not see each other's states: the buffer stays in flight
            // and this launch looks further (no buffer to be had: one chain per workgroup).
            const hipError_t q = hipEventQuery(b.done);
            if (q != hipSuccess) { (void)hipGetLastError(); continue; }
            b.in_flight = false;
        }
        chosen = i;
    }
    if (chosen < 0) {
        if (empty < 0) return nullptr;
        ScheduleBuffer& b = g_schedule_pool[empty];
        if (hipMalloc((void**)&b.flags, (size_t)kScheduleMaxChains * sizeof(unsigned)) != hipSuccess) { (void)hipGetLastError(); b.flags = nullptr; return nullptr; }
        if (hipEventCreateWithFlags(&b.done, hipEventDisableTiming) != hipSuccess || hipMemsetAsync(b.flags, 0, (size_t)kScheduleMaxChains * sizeof(unsigned), stream) != hipSuccess) {
            (void)hipGetLastError();
            if (b.done) (void)hipEventDestroy(b.done);
            (void)hipFree(b.flags);
            b = ScheduleBuffer();
            return nullptr;
        }
        b.device = device;
        b.epoch = 0;
        chosen = empty;
    }
    ScheduleBuffer& b = g_schedule_pool[chosen];
    if (b.epoch >= (1u << 30) - 1u) {                 // 4 * epoch would wrap: start over (the buffer is idle; the memset is ordered in front of the kernel)
        if (hipMemsetAsync(b.flags, 0, (size_t)kScheduleMaxChains * sizeof(unsigned), stream) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        b.epoch = 0;
    }
    b.taken = true;
    *base = 4u * ++b.epoch;
    *ticket = chosen;
    return b.flags;
}
void schedule_release(int ticket, hipStream_t stream) {
    if (ticket < 0 || ticket >= kSchedulePool) return;
    std::lock_guard<std::mutex> lock(g_schedule_mutex);
    ScheduleBuffer& b = g_schedule_pool[ticket];
    // (if the event cannot be recorded the buffer counts as idle: its last launch is then ordered only by whoever synchronises the stream)
    b.in_flight = hipEventRecord(b.done, stream) == hipSuccess;
    if (!b.in_flight) (void)hipGetLastError();
    b.taken = false;
}
}  // namespace smfft

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

void smfft_init(void) {
    read_env();
    // cudaDeviceSetCacheConfig / cudaDeviceSetSharedMemConfig (CT:579-580) have no CDNA meaning.
}

int smfft_ct_external_benchmark(const void* d_input, void* d_output, int FFT_size, int nFFTs, int inverse, int reorder, double* FFT_time) {
    return timed([&] { return dispatch_ct((const float2*)d_input, (float2*)d_output, FFT_size, nFFTs, inverse != 0, reorder != 0, 0, 0); }, FFT_time);
}

int smfft_ct_multiple_benchmark(const void* d_input, void* d_output, int FFT_size, int nFFTs, int inverse, int reorder, double* FFT_time) {
    if (nFFTs / SMFFT_NREUSES == 0) {
        if (FFT_time) *FFT_time = -1;
        return 1;
    }
    const int slots = ct_multiple_slots(FFT_size, nFFTs);
    return timed([&] { return dispatch_ct((const float2*)d_input, (float2*)d_output, FFT_size, slots, inverse != 0, reorder != 0, 1, 0); }, FFT_time);
}

int smfft_ct_multiple_unfused_benchmark(const void* d_input, void* d_output, int FFT_size, int nFFTs, int inverse, double* FFT_time) {
    if (nFFTs / SMFFT_NREUSES == 0) {
        if (FFT_time) *FFT_time = -1;
        return 1;
    }
    const int slots = ct_multiple_slots(FFT_size, nFFTs);
    return timed([&] { return dispatch_ct((const float2*)d_input, (float2*)d_output, FFT_size, slots, inverse != 0, true, 2, 0); }, FFT_time);
}

int smfft_ct_multiple_percall_benchmark(const void* d_input, void* d_output, int FFT_size, int nFFTs, int inverse, int reorder, double* FFT_time) {
    if (nFFTs / SMFFT_NREUSES == 0) {
        if (FFT_time) *FFT_time = -1;
        return 1;
    }
    const int slots = ct_multiple_slots(FFT_size, nFFTs);
    return timed([&] { return dispatch_ct((const float2*)d_input, (float2*)d_output, FFT_size, slots, inverse != 0, reorder != 0, 2, 0); }, FFT_time);
}

int smfft_st_external_benchmark(const void* d_input, void* d_output, int FFT_size, int nFFTs, double* FFT_time) {
    return timed([&] { return dispatch_st((const float2*)d_input, (float2*)d_output, FFT_size, nFFTs, 0, 0); }, FFT_time);
}
int smfft_st_external_benchmark_dir(const void* d_input, void* d_output, int FFT_size, int nFFTs, int inverse, double* FFT_time) {
    if (inverse) return smfft_st_external_benchmark(d_input, d_output, FFT_size, nFFTs, FFT_time);
    // the engine is the same autosort Stockham plan for both signs: forward natural order = Engine<N, 0, 1>
    return timed([&] { return dispatch_ct((const float2*)d_input, (float2*)d_output, FFT_size, nFFTs, false, true, 0, 0); }, FFT_time);
}
int smfft_st_multiple_benchmark(const void* d_input, void* d_output, int FFT_size, int nFFTs, double* FFT_time) {
    return timed([&] { return dispatch_st((const float2*)d_input, (float2*)d_output, FFT_size, nFFTs / SMFFT_NREUSES, 1, 0); }, FFT_time);
}

int smfft_rc_external_benchmark(const float* d_input, float* d_output, int FFT_size, int nFFTs, int inverse, double* FFT_time) {
    return timed([&] { return dispatch_rc((const float2*)d_input, (float2*)d_output, FFT_size, nFFTs, inverse != 0, 0, 0); }, FFT_time);
}
int smfft_rc_multiple_benchmark(const float* d_input, float* d_output, int FFT_size, int nFFTs, double* FFT_time) {
    return timed([&] { return dispatch_rc((const float2*)d_input, (float2*)d_output, FFT_size, nFFTs / SMFFT_NREUSES, 0, 1, 0); }, FFT_time);
}

int smfft_launch(int family, int path, const void* d_input, void* d_output, int FFT_size, int nFFTs, int inverse, int reorder, void* hip_stream) {
    read_env();
    hipStream_t st = (hipStream_t)hip_stream;
    const float2* in = (const float2*)d_input;
    float2* out = (float2*)d_output;
    if (family == 0) {
        int count = path ? ct_multiple_slots(FFT_size, nFFTs) : nFFTs;
        return dispatch_ct(in, out, FFT_size, count, inverse != 0, reorder != 0, path, st);
    }
    if (family == 1) {
        // the Stockham program is the + sign transform (ST:76); inverse = 0 asks for the forward extension, which is
        // the same autosort engine with the other sign = the natural-order CT variant (external and multiple alike)
        if (!inverse) return dispatch_ct(in, out, FFT_size, path ? nFFTs / SMFFT_NREUSES : nFFTs, false, true, path, st);
        return dispatch_st(in, out, FFT_size, path ? nFFTs / SMFFT_NREUSES : nFFTs, path, st);
    }
    if (family == 2) return dispatch_rc(in, out, FFT_size, path ? nFFTs / SMFFT_NREUSES : nFFTs, inverse != 0, path, st);
    return -1;
}

int smfft_ct_dif_external_benchmark(const void* d_input, void* d_output, int FFT_size, int nFFTs, int inverse, double* FFT_time) {
    return timed([&] { return dispatch_dif((const float2*)d_input, (float2*)d_output, FFT_size, nFFTs, inverse != 0, 0); }, FFT_time);
}

int smfft_ct_dif_launch(const void* d_input, void* d_output, int FFT_size, int nFFTs, int inverse, void* hip_stream) {
    read_env();
    return dispatch_dif((const float2*)d_input, (float2*)d_output, FFT_size, nFFTs, inverse != 0, (hipStream_t)hip_stream);
}

int smfft_copy_launch(const void* d_input, void* d_output, long long n_float2, void* hip_stream) {
    read_env();
    return smfft::launch_stream_copy((const float2*)d_input, (float2*)d_output, (long)n_float2, cur_grid_cap(), pacing_for(d_output, 16, 0), (hipStream_t)hip_stream);
}

// ---- L3 wrappers ---------------------------------------------------------------------------------
int smfft_gpu_ct(const void* h_input, void* h_output, int FFT_size, int nFFTs, int inverse, int reorder, int nRuns, double* single_ex_time, double* multi_ex_time) {
    select_device();
    // edge cases the reference rejects (CT:835-836)
    if (FFT_size == 32 && (nFFTs % 4) != 0) return 1;
    if (FFT_size == 64 && (nFFTs % 2) != 0) return 1;

    size_t free_mem, total_mem;
    checkHipErrors(hipMemGetInfo(&free_mem, &total_mem));
    if (DEBUG) printf("\n  Device has %0.3f MB of total memory, which %0.3f MB is available.\n", (float)total_mem / (1024.0 * 1024.0), (float)free_mem / (1024.0 * 1024.0));
    const size_t bytes = (size_t)FFT_size * nFFTs * sizeof(float2);
    if (!wrapper_memory_ok(bytes, 2 * bytes, free_mem)) {
        printf("Error: Not enough memory! Input data is too big for the device.\n");
        return 1;
    }
    float2 *d_input, *d_output;
    if (alloc_pair_for_wrapper(bytes, (void**)&d_input, (void**)&d_output)) checkHipErrors(hipErrorOutOfMemory);

    double time_FFT_external = 0, time_FFT_multiple = 0;
    // The reference re-uploads h_input before every one of the 2*nRuns launches (CT:868,884), outside
    // the timed region.  The kernels never modify d_input, so one upload is equivalent and saves
    // (2*nRuns - 1) pageable 4 GiB copies at the README batch.
    checkHipErrors(hipMemcpy(d_input, h_input, bytes, hipMemcpyHostToDevice));
    if (MULTIPLE) {
        if (DEBUG) printf("  Running shared memory FFT (Cooley-Tukey) 100 times per GPU kernel (eliminates device memory)... ");
        smfft_init();
        double total = 0;
        wrapper_warm_up([&](double* t) { smfft_ct_multiple_benchmark(d_input, d_output, FFT_size, nFFTs, inverse, reorder, t); });
        for (int f = 0; f < nRuns; f++) {
            smfft_ct_multiple_benchmark(d_input, d_output, FFT_size, nFFTs, inverse, reorder, &total);
        }
        time_FFT_multiple = total / nRuns;
        if (DEBUG) printf("done in %g ms.\n", time_FFT_multiple);
        if (multi_ex_time) *multi_ex_time = time_FFT_multiple;
    }
    checkHipErrors(hipGetLastError());
    if (EXTERNAL) {
        if (DEBUG) printf("  Running shared memory FFT (Cooley-Tukey)... ");
        smfft_init();
        double total = 0;
        for (int f = 0; f < nRuns; f++) {
            smfft_ct_external_benchmark(d_input, d_output, FFT_size, nFFTs, inverse, reorder, &total);
        }
        time_FFT_external = total / nRuns;
        if (DEBUG) printf("done in %g ms.\n", time_FFT_external);
        if (single_ex_time) *single_ex_time = time_FFT_external;
    }
    checkHipErrors(hipGetLastError());
    printf("  SH FFT normal = %0.3f ms; SM FFT multiple times = %0.3f ms\n", time_FFT_external, time_FFT_multiple);
    // MULTIPLE runs first, so d_output holds the EXTERNAL result (CT:862-890,898)
    checkHipErrors(hipMemcpy(h_output, d_output, bytes, hipMemcpyDeviceToHost));
    checkHipErrors(hipGetLastError());
    checkHipErrors((hipError_t)free_pair(d_input));
    return 0;
}

int smfft_gpu_st(const void* h_input, void* h_output, int FFT_size, int nFFTs, int nRuns, double* single_ex_time, double* multi_ex_time) {
    select_device();
    size_t free_mem, total_mem;
    checkHipErrors(hipMemGetInfo(&free_mem, &total_mem));
    const size_t bytes = (size_t)FFT_size * nFFTs * sizeof(float2);
    if (!wrapper_memory_ok(bytes, 2 * bytes, free_mem)) {
        printf("Error: Not enough memory! Input data is too big for the device.\n");
        return 1;
    }
    float2 *d_input, *d_output;
    if (alloc_pair_for_wrapper(bytes, (void**)&d_input, (void**)&d_output)) checkHipErrors(hipErrorOutOfMemory);
    double time_FFT_external = 0, time_FFT_multiple = 0;
    checkHipErrors(hipMemcpy(d_input, h_input, bytes, hipMemcpyHostToDevice));   // once (upstream: per run, ST:496,508)
    if (MULTIPLE) {
        smfft_init();
        double total = 0;
        wrapper_warm_up([&](double* t) { smfft_st_multiple_benchmark(d_input, d_output, FFT_size, nFFTs, t); });
        for (int f = 0; f < nRuns; f++) {
            smfft_st_multiple_benchmark(d_input, d_output, FFT_size, nFFTs, &total);
        }
        time_FFT_multiple = total / nRuns;
        if (multi_ex_time) *multi_ex_time = time_FFT_multiple;
    }
    if (EXTERNAL) {
        smfft_init();
        double total = 0;
        for (int f = 0; f < nRuns; f++) {
            smfft_st_external_benchmark(d_input, d_output, FFT_size, nFFTs, &total);
        }
        time_FFT_external = total / nRuns;
        if (single_ex_time) *single_ex_time = time_FFT_external;
    }
    checkHipErrors(hipMemcpy(h_output, d_output, bytes, hipMemcpyDeviceToHost));
    checkHipErrors(hipGetLastError());
    checkHipErrors((hipError_t)free_pair(d_input));
    printf("  SH FFT normal = %0.3f ms; SM FFT multiple times = %0.3f ms\n", time_FFT_external, time_FFT_multiple);
    return 0;
}

int smfft_gpu_r2c(void* h_output, const float* h_input, int FFT_size, int nFFTs, int nRuns) {
    select_device();
    size_t free_memory, total_memory;
    checkHipErrors(hipMemGetInfo(&free_memory, &total_memory));
    double FFT_external_time = 0, FFT_multiple_time = 0;
    const size_t input_size_bytes = (size_t)FFT_size * nFFTs * sizeof(float);
    const size_t output_size_bytes = (size_t)(FFT_size >> 1) * nFFTs * sizeof(float2);
    if (!wrapper_memory_ok(input_size_bytes, input_size_bytes + output_size_bytes, free_memory)) {
        printf("Error not enough free memory!\n");
        return 1;
    }
    float* d_input;
    float2* d_output;
    if (alloc_pair_for_wrapper(input_size_bytes, (void**)&d_input, (void**)&d_output)) checkHipErrors(hipErrorOutOfMemory);   // both sides are N*nFFTs*4 bytes
    checkHipErrors(hipMemcpy(d_input, h_input, input_size_bytes, hipMemcpyHostToDevice));
    if (MULTIPLE) {
        wrapper_warm_up([&](double* t) { smfft_rc_multiple_benchmark(d_input, (float*)d_output, FFT_size, nFFTs, t); });
        for (int r = 0; r < nRuns; r++) {
            smfft_init();
            smfft_rc_multiple_benchmark(d_input, (float*)d_output, FFT_size, nFFTs, &FFT_multiple_time);
        }
    }
    checkHipErrors(hipMemset(d_output, 0, output_size_bytes));
    if (EXTERNAL) {
        for (int r = 0; r < nRuns; r++) {
            smfft_init();
            smfft_rc_external_benchmark(d_input, (float*)d_output, FFT_size, nFFTs, 0, &FFT_external_time);
        }
    }
    printf("  smFFT R2C time: ex: %0.3f ms; mul: %0.3f ms\n", FFT_external_time / nRuns, FFT_multiple_time / nRuns);
    checkHipErrors(hipMemcpy(h_output, d_output, output_size_bytes, hipMemcpyDeviceToHost));
    checkHipErrors((hipError_t)free_pair(d_input));
    return 0;
}

int smfft_gpu_c2r(float* h_output, const void* h_input, int FFT_size, int nFFTs, int nRuns) {
    select_device();
    size_t free_memory, total_memory;
    checkHipErrors(hipMemGetInfo(&free_memory, &total_memory));
    double FFT_external_time = 0;
    const size_t input_size_bytes = (size_t)(FFT_size >> 1) * nFFTs * sizeof(float2);
    const size_t output_size_bytes = (size_t)FFT_size * nFFTs * sizeof(float);
    if (!wrapper_memory_ok(input_size_bytes, input_size_bytes + output_size_bytes, free_memory)) {
        printf("Error not enough free memory!\n");
        return 1;
    }
    float2* d_input;
    float* d_output;
    if (alloc_pair_for_wrapper(input_size_bytes, (void**)&d_input, (void**)&d_output)) checkHipErrors(hipErrorOutOfMemory);
    checkHipErrors(hipMemcpy(d_input, h_input, input_size_bytes, hipMemcpyHostToDevice));
    if (EXTERNAL) {
        for (int r = 0; r < nRuns; r++) {
            smfft_init();
            smfft_rc_external_benchmark((const float*)d_input, d_output, FFT_size, nFFTs, 1, &FFT_external_time);
        }
    }
    printf("  smFFT C2R time: ex: %0.3f ms;\n", FFT_external_time / nRuns);
    checkHipErrors(hipMemcpy(h_output, d_output, output_size_bytes, hipMemcpyDeviceToHost));
    checkHipErrors((hipError_t)free_pair(d_input));
    return 0;
}

// ---- tuning / introspection ------------------------------------------------------------------------
// the setters act on the CALLING host thread (see LaunchState above)
void smfft_set_grid_cap(int max_workgroups) { read_env(); t_state.grid_cap = max_workgroups; }
void smfft_set_nreuses(int n) { t_state.nreuses = n > 0 ? n : 0; }
int smfft_get_nreuses(void) { read_env(); return cur_nreuses(); }
int smfft_get_grid_cap(void) { read_env(); return cur_grid_cap(); }
void smfft_set_pacing(int k) { t_state.pacing = k < 0 ? -2 : k; }
void smfft_set_multiple_balance(int on) { t_state.balance = on < 0 ? -1 : on; }
int smfft_get_multiple_balance(void) { read_env(); return cur_balance(); }
void smfft_set_multiple_rotation(int log2_clocks) { t_state.rotate = log2_clocks < 0 ? -1 : log2_clocks; }
int smfft_get_multiple_rotation(void) { read_env(); return cur_rotate(); }
void smfft_set_handoff_wait_us(int microseconds) { t_state.handoff_wait_us = microseconds < 0 ? -1 : microseconds; }
void smfft_debug_delay_parking(int chain, int milliseconds, int after_commit) {
    t_state.delay_chain = milliseconds > 0 ? chain : -1;
    t_state.delay_ms = milliseconds > 0 ? milliseconds : 0;
    t_state.delay_after_commit = after_commit != 0;
}
int smfft_schedule_buffers(int* in_flight) {
    std::lock_guard<std::mutex> lock(smfft::g_schedule_mutex);
    int allocated = 0, busy = 0;
    for (const smfft::ScheduleBuffer& b : smfft::g_schedule_pool) {
        if (!b.flags) continue;
        ++allocated;
        if (b.taken || (b.in_flight && hipEventQuery(b.done) == hipErrorNotReady)) ++busy;
    }
    (void)hipGetLastError();
    if (in_flight) *in_flight = busy;
    return allocated;
}
// The most workgroups of the multiple kernel (family, FFT_size, inverse, reorder, path = 1 or 2) that are alive at once on the
// current device, COUNTED: a launch of three times what any kernel's residency can be, 60 applications each, over scratch buffers,
// with every workgroup incrementing a counter when it starts and decrementing it when it ends (workgroups of such a launch end and
// start all the time, so the count stays a few percent under what fits).  *assumed = the scheduler's figure.
int smfft_measure_multiple_residency(int family, int FFT_size, int inverse, int reorder, int path, int* assumed) {
    read_env();
    const int tile = FFT_size < 1024 ? 1024 : FFT_size;
    unsigned* counters = nullptr;
    float2 *in = nullptr, *out = nullptr;
    const int chains = 3 * 256 * 20;                       // more than any kernel's residency (at most 20 per CU), three times over for the small ones
    const size_t bytes = (size_t)chains * tile * sizeof(float2);
    if (hipMalloc((void**)&counters, 8) != hipSuccess || hipMalloc((void**)&in, bytes) != hipSuccess || hipMalloc((void**)&out, bytes) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(counters); (void)hipFree(in); (void)hipFree(out);
        return -2;
    }
    (void)hipMemset(counters, 0, 8);
    (void)hipMemset(in, 0, bytes);
    const smfft::LaunchState saved = t_state;
    t_state.balance = 0;
    t_state.nreuses = 60;
    t_state.grid_cap = 0;
    smfft::t_residency_probe = counters;
    const int count = chains * (tile / FFT_size);
    const int rc = family == 0 ? dispatch_ct(in, out, FFT_size, count, inverse != 0, reorder != 0, path, 0) : family == 1 ? dispatch_st(in, out, FFT_size, count, path, 0)
                               : dispatch_rc(in, out, 2 * FFT_size, count, inverse != 0, path, 0);      // (family 2: FFT_size = the complex length here)
    smfft::t_residency_probe = nullptr;
    t_state = saved;
    unsigned host[2] = {0, 0};
    (void)hipDeviceSynchronize();
    (void)hipMemcpy(host, counters, 8, hipMemcpyDeviceToHost);
    (void)hipFree(counters); (void)hipFree(in); (void)hipFree(out);
    if (rc != 0) return -3;
    if (assumed) *assumed = smfft::last_noted_slots();
    return (int)host[1];
}
int smfft_pacing_for_output(const void* d_output, int family, int FFT_size) {
    read_env();
    const Pacing p = family == 2 ? rc_pacing(FFT_size / 2) : c2c_pacing(FFT_size);
    return pacing_for(d_output, p.ordinary, p.mixed);
}
int smfft_device_count(void) { int n = 0; return hipGetDeviceCount(&n) == hipSuccess ? n : 0; }
int smfft_set_device(int device) { read_env(); t_state.device = device; return (int)hipSetDevice(device); }
int smfft_va_window(unsigned long long* first, unsigned long long* next) { return smfft::pairs::va_window(first, next); }
const char* smfft_version(void) { return "smfft_amd 0.1 (gfx950)"; }

int smfft_malloc_pair(unsigned long long bytes, void** d_read, void** d_written) { read_env(); return alloc_pair((size_t)bytes, d_read, d_written, true); }
int smfft_malloc_pair_for_wrapper(unsigned long long bytes, void** d_read, void** d_written) { read_env(); return alloc_pair_for_wrapper((size_t)bytes, d_read, d_written); }
int smfft_malloc_written(unsigned long long bytes, void** d_written) { read_env(); return alloc_pair((size_t)bytes, nullptr, d_written, true, -1.0, -1.0, false); }
int smfft_malloc_written_for(const void* d_read, unsigned long long bytes, void** d_written) {
    read_env();
    return alloc_pair((size_t)bytes, nullptr, d_written, true, -1.0, -1.0, false, d_read);
}
int smfft_free_written(void* d_written) { return free_pair(d_written); }
int smfft_malloc_pair_budget(unsigned long long bytes, void** d_read, void** d_written, double budget_frac, double budget_ms) {
    read_env();
    return alloc_pair((size_t)bytes, d_read, d_written, true, budget_frac, budget_ms);
}
int smfft_last_pair_info(SmfftPairInfo* out) {
    if (!out) return 1;
    smfft::pairs::last_pair_info(out);
    return 0;
}
int smfft_free_pair(void* d_read) { return free_pair(d_read); }
int smfft_pair_cache_release(void) { return smfft::pairs::release_pair_cache(-1); }
void* smfft_malloc(unsigned long long bytes) { void* p = nullptr; return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr; }
int smfft_free(void* d_ptr) { return (int)hipFree(d_ptr); }
int smfft_memcpy_h2d(void* d_dst, const void* h_src, unsigned long long bytes) { return (int)hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice); }
int smfft_memcpy_d2h(void* h_dst, const void* d_src, unsigned long long bytes) { return (int)hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost); }
int smfft_memcpy_d2d(void* d_dst, const void* d_src, unsigned long long bytes) { return (int)hipMemcpy(d_dst, d_src, bytes, hipMemcpyDeviceToDevice); }
int smfft_memset(void* d_ptr, int value, unsigned long long bytes) { return (int)hipMemset(d_ptr, value, bytes); }
int smfft_synchronize(void) { return (int)hipDeviceSynchronize(); }
int smfft_mem_info(unsigned long long* free_bytes, unsigned long long* total_bytes) {
    size_t f = 0, t = 0;
    const hipError_t rc = hipMemGetInfo(&f, &t);
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return (int)rc;
}

}  // extern "C"

// =================================================================================================
// The reference's C++-linkage names (what its FFT.c harnesses bind; include/smfft_reference_api.h)
// =================================================================================================
void FFT_init() { smfft_init(); }

int FFT_external_benchmark(float2* d_input, float2* d_output, int FFT_size, int nFFTs, bool inverse, bool reorder, double* FFT_time) {
    return smfft_ct_external_benchmark(d_input, d_output, FFT_size, nFFTs, inverse, reorder, FFT_time);
}
int FFT_multiple_benchmark(float2* d_input, float2* d_output, int FFT_size, int nFFTs, bool inverse, bool reorder, double* FFT_time) {
    return smfft_ct_multiple_benchmark(d_input, d_output, FFT_size, nFFTs, inverse, reorder, FFT_time);
}
void FFT_external_benchmark(float2* d_input, float2* d_output, int FFT_size, int nFFTs, double* FFT_time) {
    smfft_st_external_benchmark(d_input, d_output, FFT_size, nFFTs, FFT_time);
}
void FFT_multiple_benchmark(float2* d_input, float2* d_output, int FFT_size, int nFFTs, double* FFT_time) {
    smfft_st_multiple_benchmark(d_input, d_output, FFT_size, nFFTs, FFT_time);
}
void FFT_external_benchmark(float* d_input, float* d_output, int FFT_size, int nFFTs, int inverse, double* FFT_time) {
    smfft_rc_external_benchmark(d_input, d_output, FFT_size, nFFTs, inverse, FFT_time);
}
void FFT_multiple_benchmark(float* d_input, float* d_output, int FFT_size, int nFFTs, double* FFT_time) {
    smfft_rc_multiple_benchmark(d_input, d_output, FFT_size, nFFTs, FFT_time);
}

int GPU_smFFT_4elements(float2* h_input, float2* h_output, int FFT_size, int nFFTs, bool inverse, bool reorder, int nRuns, double* single_ex_time, double* multi_ex_time) {
    return smfft_gpu_ct(h_input, h_output, FFT_size, nFFTs, inverse, reorder, nRuns, single_ex_time, multi_ex_time);
}
int GPU_FFT_C2C_Stockham(float2* h_input, float2* h_smFFT_output, int FFT_size, int nFFTs, int nRuns, double* single_ex_time, double* multi_ex_time) {
    return smfft_gpu_st(h_input, h_smFFT_output, FFT_size, nFFTs, nRuns, single_ex_time, multi_ex_time);
}
int GPU_smFFT_R2C(float2* h_output, float* h_input, int FFT_size, int nFFTs, int nRuns) { return smfft_gpu_r2c(h_output, h_input, FFT_size, nFFTs, nRuns); }
int GPU_smFFT_C2R(float* h_output, float2* h_input, int FFT_size, int nFFTs, int nRuns) { return smfft_gpu_c2r(h_output, h_input, FFT_size, nFFTs, nRuns); }

// smfft_addon_host.hpp -- the host layer that the C ABI halves of the add-on libraries share (smfft_large.hip, smfft_large_real.hip,
// smfft_large_fir.hip, smfft_pfb.hip, smfft_pfb_real.hip, smfft_large_pfb.hip, smfft_pfb_spec.hip, smfft_fir_real.hip; the FIR banks through
// smfft_fir_host.hpp, which brings it to the main library's smfft_fir.hip as well; the eight row libraries through smfft_rows_host.hpp,
// which adds their grid rule, dispatch and entry point bodies): the compute units of the current device and the event-timed launch of the *_benchmark entry
// points.  Host code only, and everything has internal linkage: each library keeps a cache of its own and exports nothing from here.
#pragma once
#include <hip/hip_runtime.h>

namespace {
constexpr int kMaxDevices = 64;
int g_cus[kMaxDevices];     // compute units per device, read once

// compute units of the current device; 0 when it cannot be queried.  Devices past kMaxDevices are queried on every call.
int compute_units() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 0;
    int cus = dev < kMaxDevices ? __atomic_load_n(&g_cus[dev], __ATOMIC_RELAXED) : 0;
    if (cus <= 0) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return 0;
        if (dev < kMaxDevices) __atomic_store_n(&g_cus[dev], cus, __ATOMIC_RELAXED);
    }
    return cus;
}

// One launch on the null stream between two events, synchronous: enqueue() returns 0 or the launch's status.  Returns the first
// failing call's code; on success the elapsed milliseconds are ADDED to *FFT_time (which may be null).
template <class Enqueue>
int timed_launch(double* FFT_time, Enqueue enqueue) {
    hipEvent_t start = nullptr, stop = nullptr;
    int rc = (int)hipEventCreate(&start);
    if (rc == 0) rc = (int)hipEventCreate(&stop);
    if (rc == 0) rc = (int)hipEventRecord(start, nullptr);
    if (rc == 0) rc = enqueue();
    if (rc == 0) rc = (int)hipEventRecord(stop, nullptr);
    if (rc == 0) rc = (int)hipEventSynchronize(stop);
    float ms = 0.f;
    if (rc == 0) rc = (int)hipEventElapsedTime(&ms, start, stop);
    if (rc == 0 && FFT_time) *FFT_time += ms;
    if (start) (void)hipEventDestroy(start);
    if (stop) (void)hipEventDestroy(stop);
    return rc;
}
}  // namespace

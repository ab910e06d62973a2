// A stand-in for <hip/hip_runtime.h> on a machine's host compiler: the calls csrc/owners.hpp makes, over malloc and new, with
// counts of what is alive and a way to refuse the k-th creation (tests/cpp/owners_host.cpp).  Nothing here runs on a device.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>

struct uint4 {
    unsigned x, y, z, w;
};

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorUnknown = 999 };
enum { hipHostMallocDefault = 0, hipEventDisableTiming = 2, hipStreamNonBlocking = 1 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 };
struct ihipEvent_t { bool recorded; };
struct ihipStream_t { int priority; };
typedef ihipEvent_t *hipEvent_t;
typedef ihipStream_t *hipStream_t;

struct HipStub {
    long device = 0, pinned = 0, events = 0, streams = 0;  // alive
    long created = 0;                                      // creations of any kind asked for so far, the refused ones included
    long refuse = -1;                                      // the creation with this number (from 0) is refused; -1: none
    long refuse_copy = -1, copies = 0;                     // the same for hipMemcpyAsync
    long event_waits = 0;                                  // hipEventSynchronize calls on a recorded event
    size_t free_bytes = ~(size_t)0;                        // what hipMemGetInfo reports
    hipError_t last = hipSuccess;                          // what hipGetLastError hands out (and clears)
    long alive() const { return device + pinned + events + streams; }
    bool refused() {
        if (created++ != refuse) return false;
        last = hipErrorOutOfMemory;
        return true;
    }
};
inline HipStub g_hip;

inline const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory" : "unknown error"; }
inline hipError_t hipGetLastError() {
    const hipError_t e = g_hip.last;
    g_hip.last = hipSuccess;
    return e;
}
inline hipError_t hipMalloc(void **p, size_t n) {
    *p = nullptr;
    if (g_hip.refused()) return hipErrorOutOfMemory;
    *p = std::malloc(n ? n : 1);
    g_hip.device++;
    return hipSuccess;
}
inline hipError_t hipFree(void *p) {
    if (p) g_hip.device--;
    std::free(p);
    return hipSuccess;
}
inline hipError_t hipHostMalloc(void **p, size_t n, unsigned) {
    *p = nullptr;
    if (g_hip.refused()) return hipErrorOutOfMemory;
    *p = std::malloc(n ? n : 1);
    g_hip.pinned++;
    return hipSuccess;
}
inline hipError_t hipHostFree(void *p) {
    if (p) g_hip.pinned--;
    std::free(p);
    return hipSuccess;
}
inline hipError_t hipMemGetInfo(size_t *free_b, size_t *total_b) {
    *free_b = *total_b = g_hip.free_bytes;
    return hipSuccess;
}
inline hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) {
    *e = nullptr;
    if (g_hip.refused()) return hipErrorOutOfMemory;
    *e = new ihipEvent_t{false};
    g_hip.events++;
    return hipSuccess;
}
inline hipError_t hipEventDestroy(hipEvent_t e) {
    if (e) g_hip.events--;
    delete e;
    return hipSuccess;
}
inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t) {
    e->recorded = true;
    return hipSuccess;
}
inline hipError_t hipEventSynchronize(hipEvent_t e) {
    if (e->recorded) g_hip.event_waits++;
    return hipSuccess;
}
inline hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned, int priority) {
    *s = nullptr;
    if (g_hip.refused()) return hipErrorOutOfMemory;
    *s = new ihipStream_t{priority};
    g_hip.streams++;
    return hipSuccess;
}
inline hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned flags) { return hipStreamCreateWithPriority(s, flags, 0); }
inline hipError_t hipStreamDestroy(hipStream_t s) {
    if (s) g_hip.streams--;
    delete s;
    return hipSuccess;
}
inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
inline hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind, hipStream_t) {
    if (g_hip.copies++ == g_hip.refuse_copy) return g_hip.last = hipErrorUnknown;
    std::memcpy(dst, src, n);
    return hipSuccess;
}

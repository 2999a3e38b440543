// tests/host_abi/hip_stub.h -- the dozen HIP calls of gi_scratch.h on the host, for the sanitizer run of its failure paths (host_abi.cpp).
// TEST INFRASTRUCTURE ONLY.  Device memory is malloc / free, a "device pointer" is a host pointer, an event is a counter's value, and the
// k-th call from stub_arm(k) on fails once with hipErrorUnknown (k = 0: nothing fails).
#pragma once
#include <cstdlib>
#include <cstring>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorUnknown = 999 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
struct StubEvent { long at; };
typedef StubEvent* hipEvent_t;
typedef void* hipStream_t;

static long stub_calls = 0, stub_fail_at = 0, stub_clock = 0, stub_live_events = 0;
static inline void stub_arm(long k) { stub_calls = 0; stub_fail_at = k; }
static inline bool stub_fails() { return ++stub_calls == stub_fail_at; }

static inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "stub failure"; }
static inline hipError_t hipMalloc(void** p, size_t bytes)
{
    if (stub_fails()) { *p = (void*)0x10; return hipErrorOutOfMemory; }   // (a failed hipMalloc leaves *p undefined: the caller may not free it)
    *p = malloc(bytes);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
static inline hipError_t hipFree(void* p) { free(p); return hipSuccess; }
static inline hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind)
{
    if (stub_fails()) return hipErrorUnknown;
    memcpy(dst, src, bytes);
    return hipSuccess;
}
static inline hipError_t hipStreamSynchronize(hipStream_t) { return stub_fails() ? hipErrorUnknown : hipSuccess; }
static inline hipError_t hipEventCreate(hipEvent_t* e)
{
    if (stub_fails()) { *e = (hipEvent_t)0x10; return hipErrorUnknown; }
    *e = new StubEvent{0};
    stub_live_events++;
    return hipSuccess;
}
static inline hipError_t hipEventDestroy(hipEvent_t e) { delete e; stub_live_events--; return hipSuccess; }
static inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t)
{
    if (stub_fails()) return hipErrorUnknown;
    e->at = ++stub_clock;
    return hipSuccess;
}
static inline hipError_t hipEventSynchronize(hipEvent_t) { return stub_fails() ? hipErrorUnknown : hipSuccess; }
static inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b)
{
    if (stub_fails()) return hipErrorUnknown;
    *ms = (float)(b->at - a->at);
    return hipSuccess;
}

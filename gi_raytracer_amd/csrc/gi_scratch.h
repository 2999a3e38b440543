// gi_scratch.h -- the three things every host entry of the C ABI reaches for: device memory that frees itself (DevBuf), a pair of events
// around a pass (EventTimer) and the end of a host-pointer call (finish_to_host: drain the stream, copy the results back, name the error).
//
// Host code only, and no HIP header of its own: the includer declares the HIP calls used here first -- <hip/hip_runtime.h> in gi_kernels.hip,
// a malloc-backed stub in tests/host_abi, which drives every failure path of these helpers under the address sanitizer.
#pragma once
#include <algorithm>
#include <cstddef>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/gi_hip.h"

namespace {

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;              // one owner per allocation
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    hipError_t alloc(size_t count)               // (an empty buffer still has an address of its own)
    {
        release();
        hipError_t e = hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T));
        if (e != hipSuccess) p = nullptr;
        else n = count;
        return e;
    }
    hipError_t upload(const T* h, size_t count)
    {
        hipError_t e = alloc(count);
        if (e == hipSuccess && count) e = hipMemcpy(p, h, count * sizeof(T), hipMemcpyHostToDevice);
        return e;
    }
    hipError_t upload(const std::vector<T>& v) { return upload(v.data(), v.size()); }
    hipError_t download(T* h, size_t count) const { return count ? hipMemcpy(h, p, count * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess; }
};

// Device time of one pass: events a / b recorded around it on the pass's stream, read when somebody asks.  A call of the pass starts with reset(),
// so the time of a call that did no work, was refused or failed is 0; read() may be repeated and keeps returning the time of the last pass.
struct EventTimer {
    hipEvent_t a = nullptr, b = nullptr;
    float ms = 0;
    bool pending = false;                        // a and b were recorded and not read yet
    EventTimer() = default;
    EventTimer(const EventTimer&) = delete;      // one owner per pair of events
    EventTimer& operator=(const EventTimer&) = delete;
    ~EventTimer() { destroy(); }
    void reset() { ms = 0; pending = false; }
    hipError_t begin(hipStream_t st)
    {
        reset();
        if (!a) { hipError_t e = hipEventCreate(&a); if (e != hipSuccess) { a = nullptr; return e; } }
        if (!b) { hipError_t e = hipEventCreate(&b); if (e != hipSuccess) { b = nullptr; return e; } }
        return hipEventRecord(a, st);
    }
    hipError_t end(hipStream_t st)
    {
        const hipError_t e = hipEventRecord(b, st);
        pending = e == hipSuccess;
        return e;
    }
    hipError_t read(float* out)
    {
        if (pending) {
            hipError_t e = hipEventSynchronize(b);
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
            if (e != hipSuccess) return e;
            pending = false;
        }
        *out = ms;
        return hipSuccess;
    }
    void destroy()
    {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
        a = b = nullptr;
        reset();
    }
};

// One result of a host-pointer call: `bytes` from device memory to the caller's array; h == nullptr is an optional output nobody asked for.
struct ToHost { void* h; const void* d; size_t bytes; };
template <class T> ToHost to_host(T* h, const DevBuf<T>& d, size_t count) { return {h, d.p, count * sizeof(T)}; }

// The end of a host-pointer call whose device work is on c->stream: wait for it, copy the results back in the order given, and turn the first HIP
// error into GI_E_HIP with "<what>: <HIP's text>" as the context's message; a call that fails here has no time to report (timer: the pass's, optional).
// Ctx: anything with a stream and an err (gi_ctx).
template <class Ctx> int finish_to_host(Ctx* c, const char* what, const ToHost* outs, size_t n_outs, EventTimer* timer = nullptr)
{
    hipError_t e = hipStreamSynchronize(c->stream);
    for (size_t k = 0; k < n_outs; k++)
        if (e == hipSuccess && outs[k].h && outs[k].bytes) e = hipMemcpy(outs[k].h, outs[k].d, outs[k].bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) return GI_OK;
    if (timer) timer->reset();
    c->err = std::string(what) + ": " + hipGetErrorString(e);
    return GI_E_HIP;
}
template <class Ctx> int finish_to_host(Ctx* c, const char* what, std::initializer_list<ToHost> outs, EventTimer* timer = nullptr)
{
    return finish_to_host(c, what, outs.begin(), outs.size(), timer);
}

}  // namespace

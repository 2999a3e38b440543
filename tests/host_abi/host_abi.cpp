// tests/host_abi/host_abi.cpp -- the failure paths of the host ABI's helpers (gi_raytracer_amd/csrc/gi_scratch.h: DevBuf, EventTimer,
// finish_to_host) over a stub of HIP (hip_stub.h).  TEST INFRASTRUCTURE ONLY; built with -fsanitize=address,undefined and run on its own
// (tests/test_host_abi.py): a leak, a double free or a read of freed memory on any path ends the program with the sanitizer's report.
//
// wrapper(): the shape of a gi_*_host entry -- upload two inputs, allocate the output, run a timed device step, finish to host.  main() runs it
// with no failure, counts its HIP calls, then fails the k-th for every k and checks code, message, output and timer each time.
#include <cstdio>

#include "hip_stub.h"
#include "../../gi_raytracer_amd/csrc/gi_scratch.h"

struct Ctx { hipStream_t stream = nullptr; std::string err; EventTimer t; };

static int fail(Ctx* c, int code, const std::string& msg) { c->err = msg; return code; }
#define TRY(c, expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) return fail((c), GI_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); } while (0)

static const size_t N = 1000;

// the device step: out = a + b, between the timer's events
static int step_device(Ctx* c, const float* d_a, const float* d_b, float* d_out)
{
    c->t.reset();
    TRY(c, c->t.begin(c->stream));
    for (size_t i = 0; i < N; i++) d_out[i] = d_a[i] + d_b[i];
    TRY(c, c->t.end(c->stream));
    return GI_OK;
}
static int wrapper(Ctx* c, const float* a, const float* b, float* out, int32_t* out_opt)
{
    DevBuf<float> d_a, d_b, d_out;
    DevBuf<int32_t> d_opt;
    TRY(c, d_a.upload(a, N));
    TRY(c, d_b.upload(std::vector<float>(b, b + N)));
    TRY(c, d_out.alloc(N));
    const int rc = step_device(c, d_a.p, d_b.p, d_out.p);
    return rc != GI_OK ? rc : finish_to_host(c, "wrapper_host", {to_host(out, d_out, N), to_host(out_opt, d_opt, N)}, &c->t);
}

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "host_abi: k = %ld: %s\n", k, #cond); return 1; } } while (0)

int main()
{
    std::vector<float> a(N), b(N), out(N);
    for (size_t i = 0; i < N; i++) { a[i] = (float)i; b[i] = 0.5f; }
    long k = 0, n_calls = 0;
    {
        Ctx c;
        stub_arm(0);
        CHECK(wrapper(&c, a.data(), b.data(), out.data(), nullptr) == GI_OK);
        n_calls = stub_calls;
        for (size_t i = 0; i < N; i++) CHECK(out[i] == (float)i + 0.5f);
        float ms = -1, again = -1;
        CHECK(c.t.pending && c.t.read(&ms) == hipSuccess && ms > 0 && !c.t.pending);
        CHECK(c.t.read(&again) == hipSuccess && again == ms);         // read twice: the same time
        c.t.reset();
        CHECK(c.t.read(&ms) == hipSuccess && ms == 0);                 // a call that did no work
        c.t.destroy();
        CHECK(stub_live_events == 0);
    }
    CHECK(n_calls >= 10);                                              // 3 hipMalloc, 2 + 1 hipMemcpy, 2 hipEventCreate, 2 hipEventRecord, 1 hipStreamSynchronize
    for (k = 1; k <= n_calls; k++) {
        Ctx c;
        std::fill(out.begin(), out.end(), -1.0f);
        stub_arm(k);
        const int rc = wrapper(&c, a.data(), b.data(), out.data(), nullptr);
        CHECK(stub_calls >= k);                                        // the failure was reached
        CHECK(rc == GI_E_HIP);
        CHECK(!c.err.empty());
        CHECK(!c.t.pending);                                           // a failed call leaves no time to read ...
        stub_arm(0);
        float ms = -1;
        CHECK(c.t.read(&ms) == hipSuccess && ms == 0);                 // ... and reports 0
        CHECK(wrapper(&c, a.data(), b.data(), out.data(), nullptr) == GI_OK && out[N - 1] == (float)(N - 1) + 0.5f);   // and the context still works
        c.t.destroy();
        CHECK(stub_live_events == 0);
    }
    // the timer's own read: a failure keeps the time pending for the next read
    {
        k = 0;
        Ctx c;
        stub_arm(0);
        CHECK(c.t.begin(nullptr) == hipSuccess && c.t.end(nullptr) == hipSuccess);
        float ms = -1;
        stub_arm(1);
        CHECK(c.t.read(&ms) != hipSuccess && c.t.pending);
        stub_arm(0);
        CHECK(c.t.read(&ms) == hipSuccess && ms > 0);
        c.t.destroy();
    }
    printf("host_abi ok: %ld HIP calls, every one failed once\n", n_calls);
    return 0;
}

// The launch sequences of the one-shot device calls, written down: the table of oneshot_calls.h goes
// through the C-ABI against the mock HIP runtime with its trace on (mock_hip.cpp), single-threaded
// and with combining off, as route_trace.cpp does for the staged jobs.  After each call the number of
// records (kernel launches with grid, block, LDS bytes, stream and integer arguments; event records;
// memsets; copies with kind, bytes and stream), their hash and the kernels launched are printed;
// `oneshot_trace --full` prints every record, for a diff of two builds.
// tests/test_oneshot_trace.py compares the output byte for byte with
// tests/golden/oneshot_trace_v1.txt: a one-shot call that issues another copy or launch, or the same
// ones in another order, shows as a diff.  The mock's copies happen at once and its launches write
// nothing, so ngp_mixture_crps_mapped plans its rounds from a zeroed scan record.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "oneshot_calls.h"

extern "C" void mock_hip_trace(int on);
extern "C" void mock_hip_trace_flush(void);
extern "C" const char *mock_hip_trace_digest(long *lines, unsigned long long *hash);
extern "C" long mock_hip_errors(void);
extern "C" long mock_hip_live_allocations(void);

static int fails = 0;
static bool full = false;

static void say(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static void say(const char *fmt, ...) {
    mock_hip_trace_flush();
    va_list ap;
    va_start(ap, fmt);
    std::vprintf(fmt, ap);
    va_end(ap);
    std::printf("\n");
}
static void done() {
    if (full) return;
    long n = 0;
    unsigned long long h = 0;
    const char *kernels = mock_hip_trace_digest(&n, &h);
    say("   %ld records #%016llx: %s", n, h, kernels);
}
#define OK(call) do { const ngp_status st_ = (call); if (st_ != NGP_OK) { ++fails; say("FAIL %s -> %d", #call, (int)st_); } } while (0)

int main(int argc, char **argv) {
    full = argc > 1 && std::string(argv[1]) == "--full";
    mock_hip_trace(full ? 1 : 2);
    ngp_ctx *ctx = nullptr;
    if (ngp_ctx_create(0, &ctx) != NGP_OK) { say("FAIL no context"); return 2; }
    OK(ngp_set_combining(ctx, 0));
    OK(ngp_profile_enable(ctx, 1));
    for (const oneshot::Entry &e : oneshot::table()) {
        if (e.setup) {
            say("-- setup of %s", e.name.c_str());
            OK(e.setup(ctx));
            done();
        }
        // twice: the second call draws its blocks from what the first one gave back
        for (int rep = 0; rep < 2; ++rep) {
            say("== %s", e.name.c_str());
            OK(e.call(ctx));
            done();
        }
        if (e.teardown) e.teardown();
    }
    ngp_ctx_destroy(ctx);
    if (mock_hip_errors()) { ++fails; say("FAIL the mock runtime saw a bad free or an out-of-bounds copy"); }
    if (mock_hip_live_allocations()) { ++fails; say("FAIL device allocations left after the context was destroyed"); }
    say("oneshot_trace: %d failures", fails);
    return fails ? 1 : 0;
}

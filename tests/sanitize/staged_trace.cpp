// The launch sequences of the staged paths, written down: the sequences of staged_calls.h go through
// the C-ABI against the mock HIP runtime with its trace on (mock_hip.cpp), single-threaded and with
// combining off, as oneshot_trace.cpp does for the one-shot calls.  After each step the number of
// records (kernel launches with grid, block, LDS bytes, stream and integer arguments; event records
// and waits; memsets; copies with kind, bytes and stream), their hash, the number of streams that saw
// a launch, the number of synchronisations (the trace does not record them, and a small call pays
// about 25 us for every host round trip) and the kernels launched are printed; `staged_trace --full`
// prints every record, for a diff of two builds.  tests/test_staged_trace.py compares the output byte
// for byte with tests/golden/staged_trace_v1.txt.  The mock's copies happen at once and its launches
// write nothing: a refinement reads zero corrections and stops after its first step.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "staged_calls.h"

extern "C" void mock_hip_trace(int on);
extern "C" void mock_hip_trace_flush(void);
extern "C" const char *mock_hip_trace_digest(long *lines, unsigned long long *hash);
extern "C" long mock_hip_syncs(void);
extern "C" long mock_hip_launch_streams(void);
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

int main(int argc, char **argv) {
    full = argc > 1 && std::string(argv[1]) == "--full";
    mock_hip_trace(full ? 1 : 2);
    ngp_ctx *ctx = nullptr;
    if (ngp_ctx_create(0, &ctx) != NGP_OK) { say("FAIL no context"); return 2; }
    if (ngp_set_combining(ctx, 0) != NGP_OK || ngp_profile_enable(ctx, 1) != NGP_OK) ++fails;
    for (const staged::Sequence &q : staged::table()) {
        say("== %s", q.name.c_str());
        for (const staged::Step &s : q.steps) {
            say("-- %s", s.name.c_str());
            const long syncs = mock_hip_syncs();
            const ngp_status st = s.call(ctx);
            if (st != NGP_OK) { ++fails; say("FAIL %s -> %d", s.name.c_str(), (int)st); }
            const long waited = mock_hip_syncs() - syncs, streams = mock_hip_launch_streams();
            if (full) { say("   %ld streams, %ld synchronisations", streams, waited); continue; }
            long n = 0;
            unsigned long long h = 0;
            const char *kernels = mock_hip_trace_digest(&n, &h);
            say("   %ld records #%016llx, %ld streams, %ld synchronisations: %s", n, h, streams, waited, kernels);
        }
    }
    ngp_ctx_destroy(ctx);
    if (mock_hip_errors()) { ++fails; say("FAIL the mock runtime saw a bad free or an out-of-bounds copy"); }
    if (mock_hip_live_allocations()) { ++fails; say("FAIL device allocations left after the context was destroyed"); }
    say("staged_trace: %d failures", fails);
    return fails ? 1 : 0;
}

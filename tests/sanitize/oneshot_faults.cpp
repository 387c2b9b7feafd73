// The error paths of the one-shot device calls (the table of oneshot_calls.h) against the mock HIP
// runtime (mock_hip.cpp), built with -fsanitize=thread and with -fsanitize=address,undefined by
// tests/test_host_sanitizers.py; "0 failures" and a silent sanitizer are the test.
//   copies       for k = 1, 2, ... the k-th asynchronous copy of the call fails, until k is beyond
//                the copies the call makes: status 1 every time (the mock's error code; NGP_ERR_STATE
//                from the job a component query stages), and whenever an earlier copy of the
//                call had been queued the call synchronises AFTER the failure, before it returns (what it queued reads
//                host memory of its own frame and writes blocks that go back to the cache);
//   allocations  on a fresh context (an empty block cache), with allocations above a limit just
//                under the call's largest block failing: NGP_ERR_TOO_LARGE.
// After either failure the same context serves the same call, and after ngp_ctx_destroy nothing is
// left allocated and the runtime has seen no bad free and no out-of-bounds copy.  (The mock cannot
// show a read of a dead frame through an asynchronous copy: it copies at once.  Leaks, double
// releases and the missing synchronisation are what it can show.)
#include <cstdio>
#include <cstdlib>

#include "oneshot_calls.h"

extern "C" long mock_hip_fail_copy_after(long n);
extern "C" long mock_hip_syncs(void);
extern "C" long mock_hip_syncs_at_failed_copy(void);
extern "C" void mock_hip_set_alloc_limit(size_t bytes);
extern "C" long mock_hip_errors(void);
extern "C" long mock_hip_live_allocations(void);

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; std::printf("FAIL %s:%d ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

struct Ctx {
    ngp_ctx *c = nullptr;
    Ctx() {
        if (ngp_ctx_create(0, &c) != NGP_OK) { std::printf("FAIL no context\n"); std::exit(2); }
        (void)ngp_set_combining(c, 0);
    }
    ~Ctx() {
        ngp_ctx_destroy(c);
        CHECK(mock_hip_live_allocations() == 0, "device allocations left after the context was destroyed");
        CHECK(mock_hip_errors() == 0, "bad free / out-of-bounds copy seen by the mock runtime");
    }
};

static void copy_failures(const oneshot::Entry &e) {
    Ctx x;
    if (e.setup) CHECK(e.setup(x.c) == NGP_OK, "%s: setup", e.name.c_str());
    long k = 1;
    for (;; ++k) {
        mock_hip_fail_copy_after(k);
        const ngp_status st = e.call(x.c);
        const long left = mock_hip_fail_copy_after(0);
        if (left > 0) {                    // the call makes k - 1 copies: it ran untouched
            CHECK(st == NGP_OK, "%s: status %d without a failure", e.name.c_str(), (int)st);
            break;
        }
        CHECK(st == (k <= e.job_copies ? NGP_ERR_STATE : 1), "%s: copy %ld failed, status %d", e.name.c_str(), k, (int)st);
        if (k > 1)   // counted from the failure on: a synchronisation earlier in the call (a first round) does not serve
            CHECK(mock_hip_syncs() > mock_hip_syncs_at_failed_copy(), "%s: copy %ld failed, returned without synchronising", e.name.c_str(), k);
        CHECK(e.call(x.c) == NGP_OK, "%s: the call after copy %ld had failed", e.name.c_str(), k);
        if (k > 1000) { CHECK(false, "%s: no end of copies", e.name.c_str()); break; }
    }
    std::printf("%-44s %3ld copies\n", e.name.c_str(), k - 1);
    if (e.teardown) e.teardown();
}

// does the call fail on a fresh context when allocations above `limit` do?
static bool refused(const oneshot::Entry &e, size_t limit, bool check) {
    Ctx x;
    if (e.setup) CHECK(e.setup(x.c) == NGP_OK, "%s: setup", e.name.c_str());
    mock_hip_set_alloc_limit(limit);
    const ngp_status st = e.call(x.c);
    mock_hip_set_alloc_limit(0);
    if (check) {
        CHECK(st == NGP_ERR_TOO_LARGE, "%s: allocation above %zu bytes failed, status %d", e.name.c_str(), limit, (int)st);
        CHECK(e.call(x.c) == NGP_OK, "%s: the call after a failed allocation", e.name.c_str());
    }
    if (e.teardown) e.teardown();
    return st != NGP_OK;
}

static void allocation_failure(const oneshot::Entry &e) {
    // the largest block the call asks the runtime for: the least limit under which the call still runs
    size_t lo = 1, hi = (size_t)1 << 31;   // refused at lo, served at hi
    CHECK(refused(e, lo, false), "%s: ran without an allocation", e.name.c_str());
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        (refused(e, mid, false) ? lo : hi) = mid;
    }
    (void)refused(e, lo, true);
    std::printf("%-44s largest block %zu bytes\n", e.name.c_str(), hi);
}

int main() {
    std::vector<oneshot::Entry> calls = oneshot::table();
    for (const oneshot::Entry &e : oneshot::long_table()) calls.push_back(e);
    for (const oneshot::Entry &e : calls) {
        copy_failures(e);
        allocation_failure(e);
    }
    std::printf("oneshot_faults: %d failures\n", fails);
    return fails ? 1 : 0;
}

// The error paths of the staged runs (the sequences of staged_calls.h) against the mock HIP runtime
// (mock_hip.cpp), built with -fsanitize=thread and with -fsanitize=address,undefined by
// tests/test_host_sanitizers.py; "0 failures" and a silent sanitizer are the test.  For every step of
// every sequence, on a job the steps before it left:
//   copies       for k = 1, 2, ... the k-th asynchronous copy of the step fails, until k is beyond the
//                copies the step makes: the status is the mock's error code 1 (NGP_ERR_STATE for a
//                staging copy); whenever the step had queued anything it synchronises AFTER the
//                failure, before it returns (what it queued reads and writes host memory of the caller,
//                of its own frame and of the job); every launch record the step timed is in the
//                profile (its timer was resolved); and the SAME step on the SAME job then returns
//                NGP_OK and asks of the runtime exactly what an ordinary re-run of that step on an
//                undisturbed job asks — memsets and program upload included;
//   allocations  on a fresh context (an empty block cache), with allocations above a limit just under
//                what the step needs failing: NGP_ERR_TOO_LARGE, and the step after it succeeds.
// After ngp_ctx_destroy nothing is left allocated and the runtime has seen no bad free and no
// out-of-bounds copy.  (The mock cannot show a write into a dead frame through an asynchronous copy:
// it copies at once.  The missing synchronisation, an unresolved timer and a job left half run are
// what it can show.)
#include <cstdio>
#include <cstdlib>

#include "staged_calls.h"

extern "C" void mock_hip_trace(int on);
extern "C" const char *mock_hip_trace_digest(long *lines, unsigned long long *hash);
extern "C" long mock_hip_fail_copy_after(long n);
extern "C" long mock_hip_syncs(void);
extern "C" long mock_hip_syncs_at_failed_copy(void);
extern "C" long mock_hip_timing_events(void);
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
        (void)ngp_profile_enable(c, 1);
    }
    ~Ctx() {
        ngp_ctx_destroy(c);
        CHECK(mock_hip_live_allocations() == 0, "device allocations left after the context was destroyed");
        CHECK(mock_hip_errors() == 0, "bad free / out-of-bounds copy seen by the mock runtime");
    }
    long profiled() const {
        ngp_profile p;
        (void)ngp_profile_get(c, &p);
        long n = 0;
        for (int k = 0; k < NGP_NUM_KERNEL_CLASSES; ++k) n += (long)p.launches[k];
        return n;
    }
};

struct Digest {
    long lines = 0;
    unsigned long long hash = 0;
    bool operator==(const Digest &o) const { return lines == o.lines && hash == o.hash; }
};
static Digest digest() {
    Digest d;
    (void)mock_hip_trace_digest(&d.lines, &d.hash);
    return d;
}

static void before(const staged::Sequence &q, size_t i, ngp_ctx *c) {
    for (size_t a = 0; a < i; ++a) CHECK(q.steps[a].call(c) == NGP_OK, "%s: %s", q.name.c_str(), q.steps[a].name.c_str());
}

static void copy_failures(const staged::Sequence &q, size_t i) {
    const staged::Step &s = q.steps[i];
    const auto &rerun = s.rerun ? s.rerun : s.call;
    const char *qn = q.name.c_str(), *sn = s.name.c_str();
    Ctx x;
    // once through: every kernel of the sequence has its name in the trace, the lanes are made
    before(q, q.steps.size(), x.c);
    // the undisturbed job: what the step asks of the runtime, first and as an ordinary re-run
    before(q, i, x.c);
    (void)digest();
    CHECK(s.call(x.c) == NGP_OK, "%s: %s", qn, sn);
    const Digest first = digest();
    CHECK(rerun(x.c) == NGP_OK, "%s: %s again", qn, sn);
    const Digest again = digest();
    long k = 1;
    for (;; ++k) {
        before(q, i, x.c);
        (void)digest();
        const long timed = mock_hip_timing_events(), profiled = x.profiled();
        mock_hip_fail_copy_after(k);
        const ngp_status st = s.call(x.c);
        const long left = mock_hip_fail_copy_after(0);
        if (left > 0) {                    // the step makes k - 1 copies: it ran untouched
            CHECK(st == NGP_OK, "%s: %s: status %d without a failure", qn, sn, (int)st);
            break;
        }
        const bool queued = digest().lines > 0;
        CHECK(st == (k <= s.state_copies ? NGP_ERR_STATE : 1), "%s: %s: copy %ld failed, status %d", qn, sn, k, (int)st);
        if (queued)
            CHECK(mock_hip_syncs() > mock_hip_syncs_at_failed_copy(), "%s: %s: copy %ld failed, returned without synchronising", qn, sn, k);
        CHECK(2 * (x.profiled() - profiled) == mock_hip_timing_events() - timed,
              "%s: %s: copy %ld failed, %ld timed launch records, %ld in the profile", qn, sn, k,
              (mock_hip_timing_events() - timed) / 2, x.profiled() - profiled);
        const bool once = k <= s.once_copies;
        CHECK((once ? s.call : rerun)(x.c) == NGP_OK, "%s: %s: the step after copy %ld had failed", qn, sn, k);
        CHECK(digest() == (once ? first : again), "%s: %s: the step after copy %ld had failed is not an ordinary %s", qn, sn, k,
              once ? "first call" : "re-run");
        if (k > 1000) { CHECK(false, "%s: %s: no end of copies", qn, sn); break; }
    }
    std::printf("%-72s %-44s %3ld copies\n", qn, sn, k - 1);
    CHECK(q.steps.back().call(x.c) == NGP_OK, "%s: %s", qn, q.steps.back().name.c_str());
}

// does the step fail on a fresh context when allocations above `limit` do?
static bool refused(const staged::Sequence &q, size_t i, size_t limit, bool check) {
    const staged::Step &s = q.steps[i];
    Ctx x;
    before(q, i, x.c);
    mock_hip_set_alloc_limit(limit);
    const ngp_status st = s.call(x.c);
    mock_hip_set_alloc_limit(0);
    if (check) {
        CHECK(st == NGP_ERR_TOO_LARGE, "%s: %s: allocation above %zu bytes failed, status %d", q.name.c_str(), s.name.c_str(), limit, (int)st);
        CHECK(s.call(x.c) == NGP_OK, "%s: %s: the step after a failed allocation", q.name.c_str(), s.name.c_str());
    }
    CHECK(q.steps.back().call(x.c) == NGP_OK, "%s: %s", q.name.c_str(), q.steps.back().name.c_str());
    return st != NGP_OK;
}

static void allocation_failure(const staged::Sequence &q, size_t i) {
    size_t lo = 1, hi = (size_t)1 << 31;   // refused at lo, served at hi
    if (!refused(q, i, lo, false)) return;   // the step asks the runtime for nothing (a re-run, a fetch)
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        (refused(q, i, mid, false) ? lo : hi) = mid;
    }
    (void)refused(q, i, lo, true);
    std::printf("%-72s %-44s needs a block of %zu bytes\n", q.name.c_str(), q.steps[i].name.c_str(), hi);
}

int main() {
    mock_hip_trace(2);
    for (const staged::Sequence &q : staged::table())
        for (size_t i = 0; i + 1 < q.steps.size(); ++i) {
            copy_failures(q, i);
            allocation_failure(q, i);
        }
    std::printf("staged_faults: %d failures\n", fails);
    return fails ? 1 : 0;
}

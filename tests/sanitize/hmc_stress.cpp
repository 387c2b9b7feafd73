// ngp_grad_job_hmc against the mock HIP runtime (see mock_hip.cpp): every validation error, the
// lifetime of the job's trajectory arena (hmc, run, hmc with a longer trace, destroy; destroy
// without hmc), two threads with their own jobs on one context, a job carried by two leaves, and
// the copies in and out.  Built with -fsanitize=thread and with -fsanitize=address,undefined by
// tests/test_hmc_device_sanitizers.py; exit code 0 and a silent sanitizer are the test.  (The
// mock's kernels do nothing and its copies are memcpy: z0 / mom go up into the arena and come back
// as z1 / mom1, so what the HOST does — offsets, the gather and scatter of a two-leaf job, the
// sizes of the copies — shows as z1 == z0, mom1 == mom for every item.)
#include <atomic>
#include <cmath>
#include <cstdio>
#include <thread>
#include <vector>

#include "../../include/ngp.h"

extern "C" long mock_hip_live_allocations(void);

static std::atomic<int> fails{0};
#define CHECK(c, what) do { if (!(c)) { ++fails; std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, what); } } while (0)

struct Batch {
    int B, n;
    std::vector<int32_t> ops;
    std::vector<double> params, t, y, z0, mom;
    std::vector<ngp_kernel> k;
    std::vector<uint8_t> kind, frozen;
    size_t NL = 0;
    // items alternate: SE (stationary: the Toeplitz leaf on a regular series) and Linear (general)
    Batch(int B_, int n_, bool mixed) : B(B_), n(n_) {
        ops.resize(B);
        params.resize(3 * (size_t)B);
        k.resize(B);
        size_t po = 0;
        for (int i = 0; i < B; ++i) {
            const bool lin = mixed && (i & 1);
            ops[i] = lin ? NGP_OP_LINEAR : NGP_OP_SQEXP;
            const int np = lin ? 3 : 2;
            for (int q = 0; q < np; ++q) params[po + q] = 0.3 + 0.1 * q + 0.01 * i;
            k[i] = ngp_kernel{1, np, &ops[i], &params[po], 0.05};
            po += 3;
            for (int q = 0; q <= np; ++q) kind.push_back(q == np ? 4 : (uint8_t)(q % 5));
            NL += (size_t)np + 1;
        }
        frozen.assign(NL, 0);
        t.resize(n);
        y.resize(n);
        for (int i = 0; i < n; ++i) { t[i] = i / (double)n; y[i] = std::sin(0.3 * i); }
        z0.resize(NL);
        mom.resize(NL);
        for (size_t q = 0; q < NL; ++q) { z0[q] = 0.01 * (double)q - 0.2; mom[q] = 1.0 - 0.03 * (double)q; }
    }
};

struct Out {
    std::vector<double> z1, mom1, th, U0, K0, U1, K1, lm, trace;
    std::vector<int32_t> info;
    Out(const Batch &b, int L) : z1(b.NL, -7), mom1(b.NL, -7), th(b.NL), U0(b.B), K0(b.B), U1(b.B), K1(b.B),
                                 lm(b.B), trace((size_t)(L + 1) * b.NL), info(b.B) {}
};

static ngp_hmc_config config(int L) {
    ngp_hmc_config c{};
    c.n_leapfrog = L;
    c.eps = 0.02;
    for (int q = 0; q < 5; ++q) { c.prior_mu[q] = 0.1 * q; c.prior_sigma[q] = 1.0 + 0.1 * q; }
    return c;
}

static ngp_status hmc(ngp_grad_job *j, const Batch &b, const ngp_hmc_config &c, Out &o, bool trace,
                      bool with_frozen = true) {
    return ngp_grad_job_hmc(j, &c, b.kind.data(), with_frozen ? b.frozen.data() : nullptr, b.z0.data(),
                            b.mom.data(), o.z1.data(), o.mom1.data(), o.th.data(), o.U0.data(), o.K0.data(),
                            o.U1.data(), o.K1.data(), o.lm.data(), o.info.data(),
                            trace ? o.trace.data() : nullptr);
}

static void lifetime(ngp_ctx *ctx, int n, bool mixed, int B) {
    Batch b(B, n, mixed);
    ngp_grad_job *j = nullptr;
    CHECK(ngp_grad_stage(ctx, b.B, b.k.data(), b.n, b.t.data(), b.y.data(), 0, &j) == NGP_OK && j, "stage");
    if (!j) return;
    int32_t out5[5];
    CHECK(ngp_grad_job_info(j, out5) == NGP_OK, "info");
    if (mixed) CHECK(out5[0] > 0 && out5[2] > 0, "a mixed batch on a regular series uses both leaves");
    std::vector<double> lm(b.B), g(b.NL);
    std::vector<int32_t> info(b.B);
    Out o(b, 6);
    ngp_hmc_config c = config(3);
    CHECK(hmc(j, b, c, o, false, false) == NGP_OK, "hmc without trace");
    CHECK(o.z1 == b.z0 && o.mom1 == b.mom, "the latents of every item come back where they went up");
    CHECK(ngp_grad_job_run(j, lm.data(), g.data(), info.data()) == NGP_OK, "run after hmc");
    c = config(6);
    Out o2(b, 6);
    CHECK(hmc(j, b, c, o2, true) == NGP_OK, "hmc with a trace (the arena grows)");
    CHECK(o2.z1 == b.z0 && o2.mom1 == b.mom, "after the arena grew");
    CHECK(ngp_grad_job_set_params(j, b.params.data(), o.lm.data()) == NGP_OK, "set_params after hmc");
    c = config(2);
    CHECK(hmc(j, b, c, o2, true) == NGP_OK, "hmc with a shorter trace");
    // ---- validation: the job stays usable after every refusal
    const ngp_hmc_config good = config(2);
    ngp_hmc_config bad = good;
    bad.n_leapfrog = 0;
    CHECK(hmc(j, b, bad, o, false) == NGP_ERR_ARG, "n_leapfrog < 1");
    bad = good;
    bad.eps = NAN;
    CHECK(hmc(j, b, bad, o, false) == NGP_ERR_ARG, "eps not finite");
    bad.eps = INFINITY;
    CHECK(hmc(j, b, bad, o, false) == NGP_ERR_ARG, "eps infinite");
    bad = good;
    bad.prior_sigma[4] = 0.0;
    CHECK(hmc(j, b, bad, o, false) == NGP_ERR_ARG, "prior_sigma <= 0 for a kind in use");
    bad = good;
    bad.prior_sigma[0] = -1.0;   // kinds 0 and 1 ignore their entries
    bad.prior_sigma[1] = 0.0;
    CHECK(hmc(j, b, bad, o, false) == NGP_OK, "prior entries of kinds 0 and 1 are ignored");
    {
        Batch bk = b;
        for (int i = 0; i < bk.B; ++i) bk.k[i].ops = &bk.ops[i], bk.k[i].params = &bk.params[3 * (size_t)i];
        bk.kind[1] = 5;
        CHECK(hmc(j, bk, good, o, false) == NGP_ERR_ARG, "a kind above 4");
    }
#define NULLED(expr, what) CHECK((expr) == NGP_ERR_ARG, what)
    double *D = o.z1.data();
    int32_t *I = o.info.data();
    const uint8_t *K = b.kind.data();
    const double *Z = b.z0.data();
    NULLED(ngp_grad_job_hmc(nullptr, &good, K, nullptr, Z, Z, D, D, D, D, D, D, D, D, I, nullptr), "null job");
    NULLED(ngp_grad_job_hmc(j, nullptr, K, nullptr, Z, Z, D, D, D, D, D, D, D, D, I, nullptr), "null cfg");
    NULLED(ngp_grad_job_hmc(j, &good, nullptr, nullptr, Z, Z, D, D, D, D, D, D, D, D, I, nullptr), "null kind");
    NULLED(ngp_grad_job_hmc(j, &good, K, nullptr, nullptr, Z, D, D, D, D, D, D, D, D, I, nullptr), "null z0");
    NULLED(ngp_grad_job_hmc(j, &good, K, nullptr, Z, nullptr, D, D, D, D, D, D, D, D, I, nullptr), "null mom");
    NULLED(ngp_grad_job_hmc(j, &good, K, nullptr, Z, Z, nullptr, D, D, D, D, D, D, D, I, nullptr), "null z1");
    NULLED(ngp_grad_job_hmc(j, &good, K, nullptr, Z, Z, D, nullptr, D, D, D, D, D, D, I, nullptr), "null mom1");
    NULLED(ngp_grad_job_hmc(j, &good, K, nullptr, Z, Z, D, D, nullptr, D, D, D, D, D, I, nullptr), "null theta1");
    NULLED(ngp_grad_job_hmc(j, &good, K, nullptr, Z, Z, D, D, D, nullptr, D, D, D, D, I, nullptr), "null U0");
    NULLED(ngp_grad_job_hmc(j, &good, K, nullptr, Z, Z, D, D, D, D, nullptr, D, D, D, I, nullptr), "null K0");
    NULLED(ngp_grad_job_hmc(j, &good, K, nullptr, Z, Z, D, D, D, D, D, nullptr, D, D, I, nullptr), "null U1");
    NULLED(ngp_grad_job_hmc(j, &good, K, nullptr, Z, Z, D, D, D, D, D, D, nullptr, D, I, nullptr), "null K1");
    NULLED(ngp_grad_job_hmc(j, &good, K, nullptr, Z, Z, D, D, D, D, D, D, D, nullptr, I, nullptr), "null logml1");
    NULLED(ngp_grad_job_hmc(j, &good, K, nullptr, Z, Z, D, D, D, D, D, D, D, D, nullptr, nullptr), "null info1");
    CHECK(hmc(j, b, good, o, false) == NGP_OK, "usable after the refusals");
    // ---- the host copies follow theta1: a run after the trajectory (it reads them when it is
    // combined with company) is served, and new parameters still go in
    CHECK(ngp_grad_job_run(j, lm.data(), g.data(), info.data()) == NGP_OK, "run on the refreshed copies");
    ngp_grad_job_destroy(j);
    // a job that never ran a trajectory has no arena to free
    j = nullptr;
    CHECK(ngp_grad_stage(ctx, b.B, b.k.data(), b.n, b.t.data(), b.y.data(), 0, &j) == NGP_OK, "stage again");
    ngp_grad_job_destroy(j);
}

static void worker(ngp_ctx *ctx, int id) {
    for (int r = 0; r < 6; ++r) lifetime(ctx, id ? 70 : 21, false, 5 + 3 * id);
}

int main() {
    ngp_ctx *ctx = nullptr;
    if (ngp_ctx_create(0, &ctx) != NGP_OK) { std::printf("no context\n"); return 1; }
    lifetime(ctx, 21, false, 6);
    lifetime(ctx, 300, false, 4);
    ngp_set_batch_invariant(ctx, 1);     // route by the item alone: both leaves at any batch size
    lifetime(ctx, 320, true, 7);
    ngp_set_batch_invariant(ctx, 0);
    std::thread a(worker, ctx, 0), b(worker, ctx, 1);
    a.join();
    b.join();
    ngp_ctx_destroy(ctx);
    CHECK(mock_hip_live_allocations() == 0, "device memory left behind");
    std::printf("%d failures\n", fails.load());
    return fails.load() ? 1 : 0;
}

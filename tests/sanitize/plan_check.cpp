// The planner of the short-series launch (small_plan, csrc/ngp_plan.h) over every geometry it can
// be asked about: whatever it accepts must fit the kernel's fixed resources — twenty register blocks
// per wave (seven workers in a main sweep, eight waves otherwise), SM_MAX_PANEL panel blocks in LDS,
// at most SM_MAX_SWEEPS sweeps — and must carry every aux row-block exactly once; the inverse phase of
// a gradient job must give every block column to one wave.  Then the other route rules of
// csrc/ngp_plan.h over their whole domain, for the relations the host layer relies on
// (check_routes), the acceptance rule of lattice dates (check_lattice), the working blocks of a
// gradient leaf's run against the formulas they replaced (check_leaf_blocks) and the rule that sends
// an item to the Toeplitz leaf (check_leaf_rule).  Host code only (hipcc --cuda-host-only).
#include <cstddef>
#include <cstdio>
#include <random>
#include <vector>

#include "../../nowcastautogp_amd/csrc/ngp_internal.h"

using namespace ngp;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { ++failures; printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } while (0)

static int col_count(const SmallSweep &sw, int nbe, int k) {
    const int cm = sw.main == 1 ? nbe - 1 - k : 0;
    const int ci = std::max(std::min(sw.i1, k + 1) - sw.i0, 0);
    return cm + ci + (sw.a1 - sw.a0);
}

// tests/sanitize/mock_hip.cpp checksums the geometry argument of a launch as 128 raw bytes.  That is
// deterministic because the struct has no implicit padding (26 x int32, a double, two int64: the odd
// int32 is the explicit pad_) and every JobGeom of the host layer starts as JobGeom g{}.
static_assert(offsetof(ChunkPtrs, n_fill_chain) == 168 && offsetof(ChunkPtrs, fill_base) == 180,
              "mock_hip.cpp trace_args reads the fill counts and fill_base of a ChunkPtrs at 168 .. 184");
static_assert(sizeof(JobGeom) == 128, "mock_hip.cpp trace_args reads 128 bytes of a JobGeom");

static JobGeom value_geom(int nb0, int naux) {
    JobGeom g{};
    g.n0 = nb0 * NB;
    g.nb0 = nb0;
    g.n_real = g.n0;
    g.naux = naux;
    g.naux_pad = (naux + NB - 1) / NB * NB;
    g.short_series = 1;
    return g;
}

static void check_routes() {
    // stage_general sets JobGeom::toep from stores_structured: a job that small_job takes stores every
    // tile, and every value geometry of up to SM_MAX_NB block columns has a plan (the rule is the
    // block count's alone)
    for (int nb0 = 0; nb0 <= 8; ++nb0)
        for (int naux = 1; naux <= NGP_MAX_AUX; naux += (nb0 ? 1 : 191))
            for (int P : {1, SM_MAX_ITEMS, SM_MAX_ITEMS + 1})
                for (int flags = 0; flags < 8; ++flags) {
                    JobGeom g = value_geom(nb0, naux);
                    g.short_series = flags & 1;
                    g.invariant = (flags >> 1) & 1;
                    const int prec = (flags & 4) ? NGP_PREC_MIXED : NGP_PREC_F64;
                    const bool st = stores_structured(g, P, true, prec);
                    CHECK(!(st && small_job(g, P)), "nb0 %d naux %d P %d: structured and one launch", nb0, naux, P);
                    CHECK(!stores_structured(g, P, false, prec), "structured with the option off");
                    const bool by_count = g.short_series && nb0 <= SM_MAX_NB && (P <= SM_MAX_ITEMS || g.invariant);
                    if (nb0 >= 1) CHECK(small_job(g, P) == by_count, "nb0 %d naux %d P %d flags %d: small_job is not the block count's rule", nb0, naux, P, flags);
                    CHECK(st == (prec != NGP_PREC_MIXED && !(nb0 >= 1 && by_count)), "nb0 %d P %d flags %d: stores_structured", nb0, P, flags);
                }
    for (int nb0 = 1; nb0 <= 254; ++nb0)
        for (int bc : {1, 63, 64, 512, 513, 4096, 4097})
            for (int flags = 0; flags < 16; ++flags) {
                JobGeom g = value_geom(nb0, 7);
                g.invariant = flags & 1;
                g.aux_identity = (flags >> 1) & 1;
                const bool mixed = flags & 4, half = flags & 8;
                if (splitk_eligible(g, bc, mixed, half))
                    CHECK(!g.invariant && !mixed && !half && !g.aux_identity && bc <= SPLITK_MAX_ITEMS, "split-k of nb0 %d bc %d flags %d", nb0, bc, flags);
                if (two_lane(g, bc, mixed, half))
                    CHECK(bc <= AHEAD_EARLY_MAX_ITEMS && ahead_early(bc) && bc / 2 >= 1 && !mixed && !half, "two lanes of nb0 %d bc %d flags %d", nb0, bc, flags);
                if (diag_wave(g, bc)) CHECK(!g.invariant, "wave diagonal form in an invariant job");
                const KinvRoute kr = kinv_route(g, bc);
                CHECK((kr == KINV_LDS) == (nb0 >= KINV_LDS_MIN_NB && !small_job(g, bc)), "K^-1 route of nb0 %d bc %d", nb0, bc);
                if (g.invariant && kr == KINV_SMALL) CHECK(small_job(g, bc), "an invariant job's K^-1 route follows the chunk");
                CHECK(mixed_eligible(g, NGP_PREC_MIXED) == (nb0 >= 2 && nb0 <= 129 && !g.aux_identity), "mixed range at nb0 %d", nb0);
                CHECK(!mixed_eligible(g, NGP_PREC_F64), "fp64 job taken for mixed");
            }
    // The column schedule: every block column once and in order (by construction of the loop), THIN
    // only behind a FAT step whose pre-accumulation it continues, a FULL step first when the count is
    // odd, every diag-ahead tile joined exactly where chol_diag consumes it with the k-range it covered.
    for (int nb0 = 1; nb0 <= 254; ++nb0) {
        const JobGeom g = value_geom(nb0, 7);
        int prev = -1, forked = -1, n_full = 0;
        std::vector<int> fork_at((size_t)nb0 + 2, -1);
        for (int jj = 0; jj < nb0; ++jj) {
            const ColStepPlan st = col_step(g, jj);
            CHECK(st.mode == COL_FAT || st.mode == COL_THIN || st.mode == COL_FULL, "mode");
            if (st.mode == COL_THIN) {
                CHECK(prev == COL_FAT, "nb0 %d: THIN step %d without a FAT step before it", nb0, jj);
                CHECK(st.k0_col == (jj - 1) * NB && st.k0_diag == (jj - 1) * NB, "nb0 %d: THIN step %d starts at %d / %d", nb0, jj, st.k0_col, st.k0_diag);
            } else {
                CHECK(st.k0_col == 0, "nb0 %d: step %d accumulates from %d", nb0, jj, st.k0_col);
            }
            if (st.mode == COL_FAT) CHECK(jj + 1 < nb0, "nb0 %d: FAT step %d has no second column", nb0, jj);
            if (st.mode == COL_FULL) { ++n_full; CHECK(jj == 0 || jj == nb0 - 1, "nb0 %d: FULL step at %d", nb0, jj); }
            if (st.join) {
                CHECK(forked == jj, "nb0 %d: step %d joins a tile nobody forked", nb0, jj);
                CHECK(st.k0_diag == fork_at[(size_t)jj] * NB, "nb0 %d: diag %d starts at %d, its tile covered %d", nb0, jj, st.k0_diag, fork_at[(size_t)jj] * NB);
                forked = -1;
            } else if (st.mode != COL_THIN) {
                CHECK(st.k0_diag == 0, "nb0 %d: diag %d starts at %d without a diag-ahead tile", nb0, jj, st.k0_diag);
            }
            if (st.ahead) {
                CHECK(st.mode == COL_FAT && forked < 0 && jj + 2 < nb0, "nb0 %d: fork at %d", nb0, jj);
                forked = jj + 2;
                fork_at[(size_t)jj + 2] = jj;
            }
            prev = st.mode;
        }
        CHECK(forked < 0, "nb0 %d: a diag-ahead tile is never joined", nb0);
        CHECK(n_full == ((nb0 & 1) ? 1 : 0), "nb0 %d: %d FULL steps", nb0, n_full);
    }
    // launch sizes and gradient routes
    for (long nwg = 1; nwg <= 70000; ++nwg) {
        const int sp = launch_split(nwg);
        CHECK(sp == 4 || sp == 2 || sp == 1, "split");
        CHECK(launch_split(nwg + 1) <= sp, "split grows with the launch");
        CHECK(tiles_per_wg(nwg) == 1 || sp == 1, "four tiles per workgroup in a launch that is cut finer");
    }
    for (int B = 1; B <= 600; ++B)
        for (int n : {128, 1023, 1024, 8192})
            for (int inv = 0; inv < 2; ++inv) {
                const GradBatchRoute r = grad_batch_route(B, n, inv != 0);
                CHECK((r == GRAD_SPLIT) == (B >= SPLIT_MIN_ITEMS), "split of B %d", B);
                if (inv) CHECK(r != GRAD_UNSPLIT, "an invariant batch routed by its size");
            }
    for (int ops = 1; ops <= NGP_MAX_OPS; ++ops) {
        CHECK(grad_bucket(ops) >= 0 && grad_bucket(ops) < GRAD_BUCKETS, "bucket of %d", ops);
        CHECK(ops == 1 || grad_bucket(ops) >= grad_bucket(ops - 1), "buckets in order");
    }
    for (int groups = 1; groups <= 130; ++groups)
        for (int bc : {1, 64, 512})
            for (int nchunks = 0; nchunks <= 512; nchunks += 8)
                CHECK(splitk_count(groups, nchunks, bc) * groups <= SPLITK_SLOTS || splitk_count(groups, nchunks, bc) <= 1,
                      "split-k pieces of %d groups exceed the slots", groups);
}

// ---- detect_lattice ------------------------------------------------------------------------------------
// Whatever it accepts is read from tables at |q_i - q_j| h in place of t_i - t_j, so acceptance has to
// mean max_ij |(t_i - t_j) - (q_i - q_j) h| <= LATTICE_FIT eps span: the table arguments are the date
// differences to rounding at the scale of the differences.  The multiple is measured, not chosen: the
// worst value the two [0, 1] families (k / (n - 1) and 7 k / (7 (n - 1)), n = 2 .. 4096) show is
// LATTICE_FIT_MEASURED, and four times that is allowed to every accepted series (the rule itself
// stops at LATTICE_FIT_ACCEPT = 2.5, ngp_plan.h: below this bound, above the 2 that correctly rounded
// dates with their origin inside the span can reach).
// (In long double, the fp64 dates and h taken as exact: e_i = t_i - q_i h, max_ij = max e - min e.)
constexpr double LATTICE_FIT_MEASURED = 0.73;     // eps span; printed by every run ("worst fit")
constexpr double LATTICE_FIT = 4.0 * LATTICE_FIT_MEASURED;
static_assert(LATTICE_FIT_ACCEPT < LATTICE_FIT, "the rule accepts more than the sweep allows");
constexpr double EPS = 2.220446049250313e-16;

// fit of an accepted series in units of eps span, -1: refused
static double lattice_fit(const std::vector<double> &t) {
    double h = 0.0;
    std::vector<int32_t> q;
    int R = 0;
    if (!detect_lattice(t, &h, &q, &R)) return -1.0;
    long double lo = 0, hi = 0, tmin = t[0], tmax = t[0];
    int qmax = 0;
    for (size_t i = 0; i < t.size(); ++i) {
        const long double e = (long double)t[i] - (long double)q[i] * (long double)h;
        if (i == 0 || e < lo) lo = e;
        if (i == 0 || e > hi) hi = e;
        tmin = std::min<long double>(tmin, t[i]);
        tmax = std::max<long double>(tmax, t[i]);
        qmax = std::max(qmax, (int)q[i]);
        CHECK(q[i] >= 0 && q[i] < R, "index %d outside a table of %d", (int)q[i], R);
    }
    CHECK(qmax == R - 1, "the table has %d entries, the largest index is %d", R, qmax);
    return (double)((hi - lo) / ((long double)EPS * (tmax - tmin)));
}

static void check_lattice() {
    double worst_unit = 0.0, worst_any = 0.0;
    int accepted[6] = {}, total = 0;
    std::mt19937_64 rng(7);
    std::vector<double> t;
    auto family = [&](int n, int f, int k) -> double {
        switch (f) {
            case 0: return (double)k / (double)(n - 1);                     // unit
            case 1: return (7.0 * k) / (7.0 * (n - 1));                     // days over the last day
            case 2: return 19000.0 + 7.0 * k;                               // whole days, weekly
            case 3: return 2020.0 + (double)k / 52.0;                       // decimal years
            case 4: return 100.0 + (double)k / (double)(n - 1);
            case 5: return 1e4 + (double)k / (double)(n - 1);
            case 6: return -1.0 + 0.3 * (double)k / (double)(n - 1);
            default: return (double)k / (double)(n - 1 - (n - 1) / 9);      // forecasts beyond 1 (n >= 10: up to 1.125)
        }
    };
    for (int n = 2; n <= 4096; ++n) {
        ++total;
        for (int f = 0; f < 8; ++f) {
            t.resize((size_t)n);
            for (int k = 0; k < n; ++k) t[(size_t)k] = family(n, f, k);
            const double fit = lattice_fit(t);
            if (f <= 2 || f == 7) {
                CHECK(fit >= 0.0, "family %d refused at n = %d", f, n);
                if (f <= 1) worst_unit = std::max(worst_unit, fit);
            }
            if (fit >= 0.0 && f < 6) ++accepted[f];
            worst_any = std::max(worst_any, fit);
            CHECK(fit <= LATTICE_FIT, "family %d, n = %d: accepted with a fit of %.2f eps span", f, n, fit);
        }
        // descending whole days and daily steps from another origin
        for (int k = 0; k < n; ++k) t[(size_t)k] = 738000.0 - (double)k;
        CHECK(lattice_fit(t) == 0.0, "descending whole days at n = %d", n);
        if (n % 16 && n > 2) continue;
        // a random sparse subset of a fine lattice on either side of the table-cost refusal, in the
        // shifted conventions as well; then a random nudge of one date
        for (int rep = 0; rep < 4; ++rep) {
            const int Q = 16 * n + 4096 + (rep & 1 ? 8 : -8);
            std::vector<int> idx((size_t)n);
            for (int k = 0; k < n; ++k) idx[(size_t)k] = (int)(rng() % (uint64_t)(Q + 1));
            idx[0] = 0; idx[1] = Q; if (n > 2) idx[2] = 1;
            const double origin = rep & 2 ? 2020.0 : 0.0;
            for (int k = 0; k < n; ++k) t[(size_t)k] = origin + (double)idx[(size_t)k] / (double)Q;
            double fit = lattice_fit(t);
            if (n > 2) CHECK((rep & 1) ? fit < 0.0 : true, "n = %d: a table of %d entries accepted", n, Q + 1);
            if (n > 2 && !(rep & 1) && origin == 0.0) CHECK(fit >= 0.0, "n = %d: a sparse lattice of %d steps refused", n, Q);
            worst_any = std::max(worst_any, fit);
            CHECK(fit <= LATTICE_FIT, "sparse, n = %d rep %d: fit %.2f eps span", n, rep, fit);
            for (int k = 0; k < n; ++k) t[(size_t)k] = family(n, rep & 2 ? 3 : 0, k);
            const size_t j = (size_t)(rng() % (uint64_t)n);
            const double mag = std::pow(10.0, -16.0 + 9.0 * (double)(rng() % 1000) / 1000.0);   // 1e-16 .. 1e-7 of the span
            t[j] += mag * (t[(size_t)n - 1] - t[0]);
            fit = lattice_fit(t);
            worst_any = std::max(worst_any, fit);
            CHECK(fit <= LATTICE_FIT, "nudged by %.1e of the span, n = %d rep %d: fit %.2f eps span", mag, n, rep, fit);
        }
    }
    CHECK(worst_unit <= LATTICE_FIT_MEASURED && worst_unit > 0.5 * LATTICE_FIT_MEASURED,
          "the measured fit of the [0, 1] families is %.3f eps span, the constant says %.3f", worst_unit, LATTICE_FIT_MEASURED);
    printf("lattice sweep: %d lengths, worst fit of the [0, 1] families %.3f eps span, of anything accepted %.3f; "
           "accepted: unit %d, days/last %d, whole days %d, decimal years %d, 100 + u %d, 1e4 + u %d\n",
           total, worst_unit, worst_any, accepted[0], accepted[1], accepted[2], accepted[3], accepted[4], accepted[5]);
}

// ---- the working blocks of a gradient leaf's run (leaf_run_blocks) ----------------------------------------
// The list against the two formulas it replaced, written out as they stood: the per-item estimate of
// the chunk size (it fixes the chunk, hence the launch grids, of every geometry) and the requests of
// a chunk of Bc items, in their order.  This is the one place where the old expressions survive.
static void check_leaf_blocks() {
    long points = 0;
    for (int nb0 = 1; nb0 <= 40; ++nb0)
        for (int n_real : {64 * nb0 - 63, 64 * nb0 - 1, 64 * nb0})
            for (int lat = 0; lat < 9; ++lat)          // 0: off the lattice; 1 .. 8: maxstat, maxcp, R
                for (int flags = 0; flags < 4; ++flags)
                    for (int Bc : {1, 3, 24, 64, 513, 5000, 65535}) {
                        const bool tp = flags & 1;
                        JobGeom g{};
                        g.B = Bc + 3;
                        g.n0 = nb0 * NB;
                        g.nb0 = nb0;
                        g.n_real = n_real;
                        g.naux_pad = tp ? NB : g.n0 + NB;
                        g.item_stride = (int64_t)(g.n0 + g.naux_pad) * g.n0;
                        g.npts = g.n0;
                        g.invariant = (flags >> 1) & 1;
                        g.lattice = lat ? 1 : 0;
                        g.maxstat = (lat - 1) & 1 ? 5 : 1;
                        g.maxcp = (lat - 1) & 2 ? 5 : 1;
                        g.R = lat ? ((lat - 1) & 4 ? 300 : 1) : 0;
                        ++points;
                        // the formulas of the code this list replaced
                        const int GP = NGP_MAX_PARAMS + 1, ntri = g.nb0 * (g.nb0 + 1) / 2, nd = (g.n_real + 255) / 256;
                        const size_t l_bytes = (size_t)g.item_stride * 8;
                        const size_t tab_bytes = g.lattice ? 8 * (size_t)g.maxstat * g.R : 0;
                        const size_t sig_bytes = g.lattice ? 8 * (size_t)g.maxcp * g.npts : 0;
                        const size_t aux_bytes = 8 * (size_t)g.naux_pad * g.n0;
                        const size_t item_bytes =
                            tp ? l_bytes + 4 * tab_bytes + sig_bytes + 8 * (size_t)NB * NB * g.nb0 + aux_bytes +
                                     8 * (size_t)g.n0 + 8 * (size_t)nd * GP
                               : l_bytes + 4 * tab_bytes + sig_bytes + 8 * (size_t)g.n0 * g.n0 +
                                     8 * (size_t)g.n0 + 8 * (size_t)ntri * GP;
                        std::vector<size_t> asked;
                        asked.push_back(l_bytes * (size_t)Bc);
                        asked.push_back(8 * (size_t)Bc * NB * NB * (tp ? g.nb0 : 1));
                        if (g.lattice) {
                            asked.push_back(tab_bytes * (size_t)Bc);
                            asked.push_back(sig_bytes * (size_t)Bc);
                            asked.push_back(3 * tab_bytes * (size_t)Bc);
                        }
                        asked.push_back(tp ? aux_bytes * (size_t)Bc : 8 * (size_t)Bc * g.n0 * g.n0);
                        asked.push_back(8 * (size_t)Bc * g.n0);
                        asked.push_back(8 * (size_t)Bc);
                        asked.push_back(tp ? 8 * (size_t)Bc * nd * GP
                                           : 8 * std::max<size_t>((size_t)Bc * ntri * grad_contract_split(ntri, Bc, g.invariant != 0),
                                                                  4096) * GP);
                        asked.push_back(4 * (size_t)g.B);
                        // ... and the list
                        CHECK(leaf_item_estimate(g, tp) == item_bytes, "nb0 %d n %d lat %d flags %d: estimate %zu, was %zu",
                              nb0, n_real, lat, flags, leaf_item_estimate(g, tp), item_bytes);
                        LeafBlock b[LEAF_N_BLOCKS];
                        leaf_run_blocks(g, tp, Bc, b);
                        size_t k = 0, est = 0;
                        for (int id = 0; id < LEAF_N_BLOCKS; ++id) {
                            est += b[id].est_item;
                            if (!b[id].asked) continue;
                            CHECK(k < asked.size() && b[id].bytes == asked[k], "nb0 %d n %d lat %d flags %d Bc %d: block %d asks %zu, was %zu",
                                  nb0, n_real, lat, flags, Bc, id, b[id].bytes, k < asked.size() ? asked[k] : (size_t)0);
                            ++k;
                        }
                        CHECK(k == asked.size(), "nb0 %d lat %d: %zu requests, were %zu", nb0, lat, k, asked.size());
                        CHECK(est == item_bytes, "the estimate is not the sum of the list's per-item figures");
                    }
    printf("leaf blocks: %ld points\n", points);
}

// ---- which items take the Toeplitz leaf (toep_leaf_item, kernel_k0, series_regular) ----------------------
static void check_leaf_rule() {
    // a sum of L SqExp leaves in postfix form: 2 L - 1 operators, 2 L parameters
    auto sum_of = [](int leaves, std::vector<int32_t> *ops, std::vector<double> *par) {
        ops->clear();
        par->clear();
        for (int l = 0; l < leaves; ++l) {
            ops->push_back(NGP_OP_SQEXP);
            par->push_back(0.5);
            par->push_back(1.0);
            if (l) ops->push_back(NGP_OP_PLUS);
        }
    };
    std::vector<int32_t> ops;
    std::vector<double> par;
    auto kernel = [&](double noise) { return ngp_kernel{(int32_t)ops.size(), (int32_t)par.size(), ops.data(), par.data(), noise}; };
    sum_of(16, &ops, &par);
    CHECK(ops.size() == 31 && toep_leaf_item(kernel(0.1), 1e-5), "a stationary tree of 31 operators is refused");
    sum_of(17, &ops, &par);
    CHECK(ops.size() == 33 && !toep_leaf_item(kernel(0.1), 1e-5), "a tree of 33 operators is taken");
    static_assert(TOEP_LEAF_MAX_OPS == 31 && TOEP_LEAF_MIN_SHIFT == 1e-9, "the thresholds of the Toeplitz leaf's items");
    // Linear or ChangePoint anywhere: the general leaf
    ops = {NGP_OP_SQEXP, NGP_OP_LINEAR, NGP_OP_PLUS};
    par = {0.5, 1.0, 0.0, 0.1, 1.0};
    CHECK(!toep_leaf_item(kernel(0.1), 1e-5), "a tree with a Linear node is taken");
    ops = {NGP_OP_SQEXP, NGP_OP_SQEXP, NGP_OP_CHANGEPOINT};
    par = {0.5, 1.0, 0.5, 1.0, 0.3, 0.1};
    CHECK(!toep_leaf_item(kernel(0.1), 1e-5), "a tree with a ChangePoint node is taken");
    // the diagonal shift against k(0) = 1: exactly 1e-9 passes, the next double below does not, nor a NaN
    ops = {NGP_OP_SQEXP};
    par = {0.5, 1.0};
    CHECK(kernel_k0(kernel(0.0)) == 1.0, "k(0) of a leaf of amplitude 1");
    CHECK(toep_leaf_item(kernel(1e-9), 0.0) && toep_leaf_item(kernel(0.0), 1e-9), "a shift of exactly 1e-9 k(0) is refused");
    CHECK(!toep_leaf_item(kernel(std::nextafter(1e-9, 0.0)), 0.0), "a shift just below 1e-9 k(0) is taken");
    CHECK(!toep_leaf_item(kernel(std::nan("")), 1e-5), "a NaN noise is taken");
    // k(0) of Plus(Times(a, b), c) = |a| |b| + |c|, from the leaves' amplitudes (the last parameter of
    // each: Periodic has three, a Constant is its value), signs dropped
    ops = {NGP_OP_PERIODIC, NGP_OP_GAMMAEXP, NGP_OP_TIMES, NGP_OP_CONSTANT, NGP_OP_PLUS};
    par = {0.7, 0.25, -3.0, 0.4, 1.5, 0.5, -0.125};
    CHECK(kernel_k0(kernel(0.1)) == 3.0 * 0.5 + 0.125, "k(0) of Plus(Times(a, b), c) is %.17g", kernel_k0(kernel(0.1)));
    // a regular series: one non-zero stride over all points
    std::vector<int32_t> q(70);
    for (int i = 0; i < 70; ++i) q[(size_t)i] = 3 * i;
    CHECK(series_regular(q.data(), 70), "a stride of 3 is not regular");
    for (int i = 0; i < 70; ++i) q[(size_t)i] = 210 - 3 * i;
    CHECK(series_regular(q.data(), 70), "a descending stride is not regular");
    q[69] -= 3;
    CHECK(!series_regular(q.data(), 70), "a gap at the end is regular");
    q[69] += 3;
    q[35] += 1;
    CHECK(!series_regular(q.data(), 70), "one irregular gap is regular");
    std::fill(q.begin(), q.end(), 4);
    CHECK(!series_regular(q.data(), 70), "a stride of 0 is regular");
}

int main() {
    check_routes();
    check_lattice();
    check_leaf_blocks();
    check_leaf_rule();
    int accepted = 0, refused = 0;
    for (int grad = 0; grad < 2; ++grad)
        for (int n0 = 64; n0 <= 320; n0 += 64)
            for (int n_real = grad ? n0 - 63 : n0; n_real <= n0; ++n_real)
                for (int naux = 1; naux <= (grad ? 1 : NGP_MAX_AUX); ++naux) {
                    JobGeom g{};
                    g.n0 = n0;
                    g.nb0 = n0 / NB;
                    g.n_real = n_real;
                    g.aux_identity = grad;
                    g.naux = grad ? n0 + 1 : naux;
                    g.naux_pad = grad ? n0 + NB : (naux + NB - 1) / NB * NB;
                    g.short_series = 1;
                    SmallPlan pl{};
                    if (!small_plan(g, &pl)) {
                        ++refused;
                        CHECK(n0 > 256 || !grad, "a gradient geometry of n0 = %d, n_real = %d was refused", n0, n_real);
                        continue;
                    }
                    ++accepted;
                    CHECK(n0 <= 256, "n0 = %d accepted", n0);
                    const int nbe = pl.nbe, nb16 = n0 / 16;
                    CHECK(nbe == (n_real + 15) / 16 && nbe <= 16, "nbe %d", nbe);
                    CHECK(pl.nsweeps >= 1 && pl.nsweeps <= SM_MAX_SWEEPS, "sweeps %d", pl.nsweeps);
                    CHECK(pl.npanel <= SM_MAX_PANEL && small_lds_bytes(pl) <= 160 * 1024, "panel %d", pl.npanel);
                    CHECK(pl.sw[0].main == 1, "the first sweep factorises");
                    std::vector<int> dense(nb16 + 64, 0);
                    int n_inverse = 0;
                    for (int si = 0; si < pl.nsweeps; ++si) {
                        const SmallSweep &sw = pl.sw[si];
                        CHECK(si == 0 || sw.main != 1, "one main sweep");
                        if (sw.main == 2) {
                            ++n_inverse;
                            CHECK(grad && sw.i0 == 0 && sw.i1 == nbe, "inverse phase covers the identity rows");
                            for (int j = 0; j < nbe; ++j) {
                                const int w = (int)((pl.colwave >> (4 * j)) & 15);
                                CHECK(w >= 0 && w < SM_WAVES, "column %d on wave %d", j, w);
                            }
                            continue;
                        }
                        int blocks = 0;
                        for (int k = 0; k < nbe; ++k) blocks += col_count(sw, nbe, k);
                        const int cap = (sw.main == 1 ? SM_WAVES - 1 : SM_WAVES) * SM_NSLOT;
                        CHECK(blocks <= cap, "n0 %d n_real %d naux %d sweep %d: %d blocks > %d", n0, n_real, g.naux, si, blocks, cap);
                        CHECK(nbe + (sw.i1 - sw.i0) + (sw.a1 - sw.a0) <= pl.npanel, "panel rows of sweep %d", si);
                        for (int a = sw.a0; a < sw.a1; ++a) ++dense[(size_t)a];
                    }
                    if (grad) {
                        CHECK(n_inverse == 1, "one inverse phase");
                        CHECK(dense[(size_t)nb16] == 1, "y' row-block carried %d times", dense[(size_t)nb16]);
                    } else {
                        const int nba = (naux + 15) / 16;
                        for (int a = 0; a < nba; ++a) CHECK(dense[(size_t)a] == 1, "aux row-block %d carried %d times", a, dense[(size_t)a]);
                        for (int a = nba; a < (int)dense.size(); ++a) CHECK(dense[(size_t)a] == 0, "aux row-block %d is not there", a);
                    }
                }
    printf("%d geometries accepted, %d refused, %d failures\n", accepted, refused, failures);
    return failures ? 1 : 0;
}

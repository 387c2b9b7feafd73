// ngp_plan.h — every host-side route rule of the library, once: which launch shape a chunk gets is
// decided here, from (JobGeom, chunk size, a few flags), and nowhere else.  Plain host C++ (no HIP
// runtime calls, no device code), included by ngp_internal.h behind the structs it reads, so the
// rules can be swept on the host (tests/sanitize/plan_check.cpp) and the launch sequences they give
// are recorded (tests/sanitize/route_trace.cpp, tests/golden/route_trace_v1.txt).
// Two thresholds that are equal today keep two names where they guard different things.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

namespace ngp {

// ---- thresholds ------------------------------------------------------------------------------------
constexpr int SM_MAX_ITEMS = 4096;      // larger chunks fill the chip on the column sweep (measured: 24 x n = 208 scenarios x particles up to 4,096 items win here, 8,192 gradient items lose)
constexpr int SM_MAX_NB = 4;            // the one-launch kernel holds a main block of at most 256 points
constexpr size_t MAX_CHUNK_ITEMS = 65535;   // gridDim.y
// every MIXED_REORDER block columns the items of a mixed-precision chunk are re-ranked by the fp64
// tile products they needed since the last ranking
constexpr int MIXED_REORDER = 16;
// mixed precision needs at least one fat step (two block columns); shorter series run fp64, and
// so do series of more than 129 block columns (n > 8,319): a fat step classifies its k-tiles
// in two 64-bit masks
constexpr int MIXED_MIN_NB = 2, MIXED_MAX_NB = 129;
// "a small chunk" (the 24- and 64-particle calls of a fit), rule by rule:
constexpr int AHEAD_EARLY_MAX_ITEMS = 512;    // the diag-ahead tile goes BEFORE chol_diag / the fat step (col_step)
constexpr int SPLITK_MAX_ITEMS = 512;         // split-k fat steps of late columns
constexpr int DIAG_WAVE_MAX_ITEMS = 512;      // chol_diag_wave_kernel (diag_wave below)
constexpr int CONTRACT_TWO_STREAM_MAX_ITEMS = 512;   // size classes of the contraction alternate between two streams
constexpr int KINV_SMALL_MAX_ITEMS = 512;     // K^-1 of a series up to 448 points on the 16 x 16-block kernel
// block columns from which a series is "long": the split-k fat steps pay, and K^-1 = W W' is staged
// through LDS as 2 x 2 tile blocks (below it: the wave-per-tile form, or the 16 x 16-block kernel)
constexpr int SPLITK_MIN_NB = 8, KINV_LDS_MIN_NB = 8;
// Two lanes pay from n ~ 1500 and 64 items on (measured, 64 items: n = 2048 logml 6.78 -> 6.57 ms,
// logml + gradient 17.07 -> 16.41; n = 1024: 2.00 -> 2.20 and 4.13 -> 4.21, so not there); three and
// four lanes were slower everywhere (more streams than hardware queues).
constexpr int TWO_LANE_MIN_ITEMS = 64, TWO_LANE_MIN_NB = 24;
// diag_ahead_kernel: four waves along k from this many accumulated columns on
constexpr int DIAG_AHEAD_SPLIT_K = 512;
// split-k fat steps fill the chip to 384, not the 512 workgroups it holds: chol_diag's successor tile
// (diag_ahead, 4 waves of 224 VGPRs) is resident beside this launch and a second round costs more
// than the split saves (measured at 64 items, n = 2048)
constexpr int SPLITK_FILL_WGS = 384;
// small launches are cut finer (four, two, one workgroup per tile); very large ones take four tiles
// per workgroup
constexpr long SPLIT4_MAX_WGS = 1024, SPLIT2_MAX_WGS = 2048, TILES4_MIN_WGS = 65536;
// the contraction sorts a chunk's items by tree size only when the launches are large enough: small
// ones stay ONE launch sized by the largest tree (up to five dependent launches of a few
// microseconds each cost more there than the occupancy of the smaller instantiations gains)
constexpr long BY_SIZE_MIN_WGS = 4096, BY_SIZE_MIN_WGS_TOEP = 512;
// A gradient batch that is split runs its two leaves one after the other: two chains of dependent
// launches instead of one.  That pays when the leaves are throughput-bound (12,800 items at n = 2049:
// 2,615 -> 1,794 ms) and costs when they are latency-bound (24 items at n = 208: 615 -> 790 us; 64 at
// n = 2048: 15.9 -> 16.3 ms), so a mixed batch is split only from SPLIT_MIN_ITEMS on; a batch
// of stationary trees only is never split and always takes the Toeplitz path.
// Just below that (PAIR_MIN_ITEMS .. SPLIT_MIN_ITEMS, long series) the two leaves run SIDE BY SIDE
// on two stream pairs (grad_pair_run); smaller mixed batches are not split at all.  Measured on
// the prior ensemble at n = 2048, general job -> split: 64 items 15.1 -> 17.2 ms side by side
// (each leaf's chain is as long as the whole batch's, and they compete for the chip), 128 items
// 26.8 -> 25.0 side by side, 256 items 50.2 -> 40.0 and 512 items 98.8 -> 72.0 in turn
// (scripts/mixed_grad_probe.py).
constexpr int SPLIT_MIN_ITEMS = 256, PAIR_MIN_ITEMS = 128, PAIR_MIN_N = 1024;
// the Toeplitz gradient leaf: at least two blocks, short enough for the weights kernel's LDS image
constexpr int TOEP_GRAD_MIN_N = 2 * NB, TOEP_GRAD_MAX_N = 8192;
// ... and of such a series the items it takes (toep_leaf_item): trees of at most 16 leaves, i.e. 31
// operators (the 1-D contraction runs on the register-accumulator kernels, which end there), whose
// diagonal shift noise + jitter is at least this fraction of the diagonal k(0)
constexpr int TOEP_LEAF_MAX_OPS = 31;
constexpr double TOEP_LEAF_MIN_SHIFT = 1e-9;
// stage_general / grad_leaf_stage keep a staging buffer up to this size with the job instead of
// waiting for the copy; ngp_job_fetch brings a result region up to FETCH_PACKED_BYTES back in one copy
constexpr size_t STAGE_KEEP_BYTES = (size_t)4 << 20, FETCH_PACKED_BYTES = (size_t)1 << 20;

// ---- short series in one launch --------------------------------------------------------------------
// The plan of a geometry, or false when the column sweep has to do it (n0 > 256, structured
// storage, the Toeplitz gradient path, more aux rows than four sweeps hold).
inline bool small_plan(const JobGeom &g, SmallPlan *pl) {
    if (g.n0 <= 0 || g.nb0 > SM_MAX_NB || g.aux_e1 || g.toep) return false;
    const int nb16 = g.n0 / 16, nbe = (g.n_real + 15) / 16;
    if (nbe < 1 || nbe > nb16) return false;
    const int cap_main = (SM_WAVES - 1) * SM_NSLOT, cap_aux = SM_WAVES * SM_NSLOT;
    SmallPlan p{};
    p.nbe = nbe;
    p.ident = g.aux_identity ? 1 : 0;
    int used = nbe * (nbe - 1) / 2;
    if (used > cap_main) return false;
    int ns = 0, npanel = nbe;
    if (g.aux_identity) {
        const int ytile = nb16;                           // slab rows 2 n0 ...: y'
        if (used + nbe > cap_main) return false;          // (120 + 16 <= 140)
        p.sw[ns++] = SmallSweep{1, 0, 0, ytile, ytile + 1};
        p.sw[ns++] = SmallSweep{2, 0, nbe, 0, 0};
        npanel = std::max(npanel, nbe + 1);
        // Block column j of L^-1 costs (nbe - j)(nbe - j - 1) / 2 block products, all on one wave.
        // Longest first, each to the wave whose SIMD (waves w and w + 4 share one) carries least;
        // of that SIMD's two waves the less loaded one.
        int load[SM_WAVES] = {};
        for (int j = 0; j < nbe; ++j) {
            int best = 0;
            for (int w = 1; w < SM_WAVES; ++w) {
                const int sb = load[best % 4] + load[best % 4 + 4], sw_ = load[w % 4] + load[w % 4 + 4];
                if (sw_ < sb || (sw_ == sb && load[w] < load[best])) best = w;
            }
            load[best] += (nbe - j) * (nbe - j - 1) / 2 + 1;
            p.colwave |= (uint64_t)best << (4 * j);
        }
    } else {
        const int nba = (g.naux + 15) / 16;
        int a = std::min(nba, (cap_main - used) / nbe);
        a = std::min(a, SM_MAX_PANEL - nbe);
        p.sw[ns++] = SmallSweep{1, 0, 0, 0, a};
        npanel = std::max(npanel, nbe + a);
        while (a < nba) {
            if (ns == SM_MAX_SWEEPS) return false;
            const int b = std::min(nba, a + std::min(cap_aux / nbe, SM_MAX_PANEL - nbe));
            p.sw[ns++] = SmallSweep{0, 0, 0, a, b};
            npanel = std::max(npanel, nbe + b - a);
            a = b;
        }
    }
    if (npanel > SM_MAX_PANEL) return false;
    p.nsweeps = ns;
    p.npanel = std::max(npanel, 9);     // (the waves' 16 x 18 staging corners of the prologue: 8 x 2,304 B)
    *pl = p;
    return true;
}

// the rule every caller shares: the geometry qualifies and the chunk is not one that fills the chip
// many times over (batch-invariant jobs: the geometry alone decides)
inline bool small_job(const JobGeom &g, int Bc, SmallPlan *pl = nullptr) {
    SmallPlan tmp;
    return g.short_series && small_plan(g, pl ? pl : &tmp) && (Bc <= SM_MAX_ITEMS || g.invariant);
}

// Structured storage of a staged value job (JobGeom::toep is set from this, so g.toep is still 0):
// fp64 jobs that reach the column sweep — short series are factorised from registers in one launch
// and store every tile; mixed precision keeps every tile (its shadow copies and tile maxima come
// from the stored rows)
inline bool stores_structured(const JobGeom &g, int P, bool option_on, int precision) {
    return option_on && precision != NGP_PREC_MIXED && !small_job(g, P);
}

// ---- the column sweep of one chunk -----------------------------------------------------------------
inline bool mixed_eligible(const JobGeom &g, int precision) {
    return precision == NGP_PREC_MIXED && g.nb0 >= MIXED_MIN_NB && g.nb0 <= MIXED_MAX_NB && !g.aux_identity;
}
// small chunks of long series: late block columns (few tile pairs, long k-loops) are cut along k.
// half: the chunk is one half of a two-lane sweep or one leaf of a pair (its owner reserves the buffer)
inline bool splitk_eligible(const JobGeom &g, int bc, bool mixed, bool half) {
    return !half && bc <= SPLITK_MAX_ITEMS && !mixed && !g.aux_identity && g.nb0 >= SPLITK_MIN_NB && !g.invariant;
}
// pieces of one tile pair's k-range; every piece keeps at least 8 staged chunks of the k-loop
inline int splitk_count(int groups, int nchunks, int Bc) {
    return std::min(std::min(8, SPLITK_SLOTS / std::max(groups, 1)),
                    std::min(nchunks / 8, SPLITK_FILL_WGS / std::max(groups * Bc, 1)));
}
// two half-chunks side by side, each on its own pair of streams (factor_chunk)
inline bool two_lane(const JobGeom &g, int bc, bool mixed, bool half) {
    return !half && !mixed && bc >= TWO_LANE_MIN_ITEMS && bc <= AHEAD_EARLY_MAX_ITEMS && g.nb0 >= TWO_LANE_MIN_NB;
}
// Small chunks, where the launch is on the critical path of the sweep: chol_diag_wave_kernel (42 ->
// 34 us at 64 items).  Large chunks keep chol_diag_kernel: there every workgroup competes for its CU
// with three others and what counts is its total work, of which the wave form — one wave factoring
// while three wait — has more (6,400 items: 376 -> 455 us per launch).  Batch-invariant jobs never
// switch (the two forms differ in the last bits).
inline bool diag_wave(const JobGeom &g, int Bc) { return !g.invariant && Bc <= DIAG_WAVE_MAX_ITEMS; }
// the split depends on the geometry only (not on the batch), so a given matrix is always summed in
// the same order
inline int diag_ahead_waves(int j) { return j * NB >= DIAG_AHEAD_SPLIT_K ? 4 : 1; }

// One block column of the left-looking sweep.  Block columns go in pairs: a FAT step finishes column
// jj and pre-accumulates column jj + 1 (and, on a side stream, the diagonal tile of jj + 2: `ahead`)
// from the same streamed rows; the THIN step that follows only adds k in [64 (jj - 1), 64 jj).
// An odd number of block columns: column 0 goes alone (a FULL step without a k-loop: only the
// solve) and the pairs start at column 1.  Pairing from column 0 leaves the LAST column alone,
// whose FULL step carries the longest k-loop of the sweep on the direct-load kernel (gradient
// jobs at n = 2049, 33 block columns: 62 MB of reads per item and 3.7 % of the call).
struct ColStepPlan {
    int mode;      // COL_FAT / COL_THIN / COL_FULL
    int k0_col;    // first k the column step still has to accumulate
    // diag tile (jj, jj): second column of a pair: pre-accumulated over k < 64 (jj - 1) by the fat
    // step jj - 1; first column of the second pair on: over k < 64 (jj - 2) by its diag-ahead tile
    int k0_diag;
    bool ahead;    // launches the diag-ahead tile (jj + 2, jj + 2) on the side stream
    bool join;     // the diag-ahead tile (jj, jj), launched at step jj - 2, is joined before chol_diag(jj)
};
inline int col_pair_offset(const JobGeom &g) { return (g.nb0 >= 3 && (g.nb0 & 1)) ? 1 : 0; }
inline ColStepPlan col_step(const JobGeom &g, int jj) {
    const int o = col_pair_offset(g);
    const bool fat = jj >= o && ((jj - o) % 2 == 0) && (jj + 1 < g.nb0);
    const bool thin = jj >= o && ((jj - o) % 2 == 1);
    ColStepPlan st;
    st.mode = fat ? COL_FAT : (thin ? COL_THIN : COL_FULL);
    st.k0_col = thin ? (jj - 1) * NB : 0;
    st.k0_diag = thin ? (jj - 1) * NB : (jj - o >= 2 ? (jj - 2) * NB : 0);
    st.ahead = fat && jj + 2 < g.nb0 && jj > 0;
    // (the tile (jj, jj) was forked by the fat step jj - 2, which had to exist, be fat and not be column 0)
    st.join = (jj - o) % 2 == 0 && jj - 2 >= std::max(o, 1);
    return st;
}
// Small chunks: the diag-ahead tile of a pair goes to the side stream BEFORE chol_diag / the fat step
// — everything it reads (rows of block jj + 2, columns < 64 jj) is final once column jj - 1 is.
// Beside the fat step it has several hundred microseconds to hide in; launched after it (the order
// of large chunks: beside chol_diag(jj + 1) / the thin step of jj + 1 — beside the fat step it cost
// more there, profiles/r02/README.md) its single-wave k-loop outlasts chol_diag + the thin step from
// n ~ 1500 on and chol_diag(jj + 2) waits for it.  The order of launches does not change any result.
inline bool ahead_early(int bc) { return bc <= AHEAD_EARLY_MAX_ITEMS; }

// ---- launch sizes ------------------------------------------------------------------------------------
// workgroups per 64 x 64 tile of a fill or contraction launch of nwg tiles
inline int launch_split(long nwg) { return nwg <= SPLIT4_MAX_WGS ? 4 : (nwg <= SPLIT2_MAX_WGS ? 2 : 1); }
inline int tiles_per_wg(long nwg) { return nwg >= TILES4_MIN_WGS ? 4 : 1; }

// ---- lattice dates -----------------------------------------------------------------------------------
// Do all dates sit on a lattice t = tmin + q h (integer-day dates, before or after a rescale)?  Every
// consumer of "lattice" dates trusts this one decision: once a series is accepted, a stationary
// subtree is no longer evaluated at t_i - t_j but read from a table at |q_i - q_j| h.
// Floating-point Euclid over the gaps gives h; then the residuals e_i = (t_i - tmin) - q_i h, formed
// without rounding error (two-sum and fma), must all lie within LATTICE_FIT_ACCEPT eps span of each
// other: max_ij |(t_i - t_j) - (q_i - q_j) h| <= 2.5 eps (tmax - tmin), so a table argument equals the
// difference of the dates to rounding AT THE SCALE OF THE DIFFERENCES.  Correctly rounded dates on a
// lattice whose origin is within the span of the data (max |t| <= span: k / (n - 1) with forecasts
// beyond 1, slope (days - origin), whole-day numbers, which are exact) fit within 2: eps / 2 |t_i| from
// each date and eps / 2 span from h = span / qmax.  tests/sanitize/plan_check.cpp sweeps the rule.
// The bound is NOT taken at the magnitude of the dates (it was: 16 eps max(|t|, 1) per point).  Dates
// far from their origin (decimal years 2020 + k / 52, 1e4 + k / (n - 1)) carry a representation noise
// of eps |t| / 2 each, many eps of the span, and tables built on them were off by up to 4e-10 k(0)
// per entry (logml of a 321-point series by 9e-10 relative, on the device).  Such dates are refused
// and evaluated directly, which is right to rounding for any dates and slower; a caller who wants
// the tables subtracts the origin first (whole-day dates minus a whole-day origin are exact).
constexpr double LATTICE_FIT_ACCEPT = 2.5, LATTICE_SNAP = 1e-9;
constexpr int LATTICE_MAX_STEPS = 1 << 20;
inline bool detect_lattice(const std::vector<double> &t, double *h_out, std::vector<int32_t> *q,
                           int *R_out) {
    const size_t n = t.size();
    if (n < 2) return false;
    double tmin = t[0], tmax = t[0];
    for (double v : t) { tmin = std::min(tmin, v); tmax = std::max(tmax, v); }
    if (!(tmax > tmin) || !std::isfinite(tmax) || !std::isfinite(tmin)) return false;
    const double span = tmax - tmin;
    const double tol = LATTICE_SNAP * span;
    double g = 0.0;
    for (double v : t) {
        double a = v - tmin;
        if (a <= tol) continue;
        if (g == 0.0) { g = a; continue; }
        double x = g, y = a;          // Euclid with snapping
        for (int it = 0; it < 64 && y > tol; ++it) {
            double r = std::fmod(x, y);
            if (y - r <= tol) r = 0.0;
            x = y;
            y = r;
        }
        g = x;
        if (g < span / (double)LATTICE_MAX_STEPS) return false;
    }
    if (g <= 0.0) return false;
    const double qmaxd = std::round(span / g);
    if (qmaxd < 1.0 || qmaxd > (double)LATTICE_MAX_STEPS) return false;
    // a lattice far sparser than the data (a few points on a very fine grid) would cost more in
    // tables (R entries per stationary subtree and item) than direct evaluation costs in the fill
    if (qmaxd > 16.0 * (double)n + 4096.0) return false;
    const double h = span / qmaxd;
    q->resize(n);
    double lo = 0.0, hi = 0.0;
    for (size_t i = 0; i < n; ++i) {
        const double a = t[i] - tmin, bv = a - t[i];
        const double a_err = (t[i] - (a - bv)) + (-tmin - bv);      // t_i - tmin = a + a_err exactly
        const double qi = std::round(a / h);
        const double e = std::fma(-qi, h, a) + a_err;
        lo = i ? std::min(lo, e) : e;
        hi = i ? std::max(hi, e) : e;
        if (hi - lo > LATTICE_FIT_ACCEPT * 2.220446049250313e-16 * span) return false;
        (*q)[i] = (int32_t)qi;
    }
    *h_out = h;
    *R_out = (int)qmaxd + 1;
    return true;
}

// ---- the fill ----------------------------------------------------------------------------------------
enum FillRoute {
    FILL_DIRECT,        // no lattice: every entry evaluated from the dates (fill_kernel)
    FILL_GRAD_SMALL,    // short gradient job: ONE launch on the full program, main tiles only
    FILL_GRAD_LISTS,    // gradient job: main tiles through the value kernels by program shape, then the aux tiles
    FILL_GRAD_FULL,     // gradient job without fill lists / aux rows only: the full program
    FILL_VALUE_LISTS,   // staged value job: other / chain / single-table items on their own kernels
    FILL_VALUE_ONE      // ONE launch on the general kernel (short jobs, resident factors' aux rows, no lists)
};
// Short jobs are chains of launches a few microseconds long: ONE fill launch on the general kernel
// (reduced / full programs; the chain and single-table kernels compute the same values, operation
// for operation) instead of up to three per program shape plus the aux one
inline FillRoute fill_route(const JobGeom &g, bool grad_tables, bool has_lists, int Bc, bool aux_only) {
    if (!g.lattice) return FILL_DIRECT;
    const bool one_launch = small_job(g, Bc);
    if (one_launch && grad_tables && !aux_only) return FILL_GRAD_SMALL;
    if (grad_tables && has_lists && !aux_only) return FILL_GRAD_LISTS;
    if (grad_tables) return FILL_GRAD_FULL;
    if (has_lists && !aux_only && !one_launch) return FILL_VALUE_LISTS;
    return FILL_VALUE_ONE;
}

// ---- gradient jobs -----------------------------------------------------------------------------------
// K^-1 = W W' of the general leaf: short jobs (factor_chunk's rule), and small chunks of series up to
// 448 points on the column sweep — its W_I has the same entries where the 16 x 16-block kernel reads
// them; long series stage 2 x 2 tile blocks through LDS (HBM traffic halves against the
// wave-per-tile form)
enum KinvRoute { KINV_SMALL, KINV_WAVE, KINV_LDS };
inline bool kinv_lds(const JobGeom &g) { return g.nb0 >= KINV_LDS_MIN_NB; }
inline KinvRoute kinv_route(const JobGeom &g, int bc) {
    if (small_job(g, bc) || (!kinv_lds(g) && bc <= KINV_SMALL_MAX_ITEMS && !g.invariant)) return KINV_SMALL;
    return kinv_lds(g) ? KINV_LDS : KINV_WAVE;
}
// items / bucket_counts of the contraction launchers: the chunk's items sorted by tree size into
// GRAD_BUCKETS groups — at most 1, 2, 4, 8, 16 leaves, larger
constexpr int GRAD_BUCKETS = 6;
inline int grad_bucket(int n_ops) {
    return n_ops <= 1 ? 0 : n_ops <= 3 ? 1 : n_ops <= 7 ? 2 : n_ops <= 15 ? 3 : n_ops <= 31 ? 4 : 5;
}
// every size class on the contraction kernel sized for it?  (batch-invariant jobs: always — an item
// then runs on the instantiation of ITS tree size, not on the one the largest tree of its batch picks)
inline bool contract_by_size(const JobGeom &g, bool toep_path, int bc) {
    const int ntri = g.nb0 * (g.nb0 + 1) / 2, nd = (g.n_real + 255) / 256;
    return g.lattice && (g.invariant || (toep_path ? (long)nd * bc > BY_SIZE_MIN_WGS_TOEP
                                                   : (long)ntri * bc > BY_SIZE_MIN_WGS));
}
// size classes of a SMALL chunk alternate between the main and the side stream: each is a few
// rounds of the chip with a ragged last one, and they touch different items
inline bool contract_two_streams(int Bc) { return Bc <= CONTRACT_TWO_STREAM_MAX_ITEMS; }
// workgroups per 64x64 tile of the gradient contraction: small launches are cut finer
// (batch-invariant jobs: by the geometry alone — the split decides how a thread groups its rows,
// i.e. the order of a partial sum)
inline int grad_contract_split(long ntri, long Bc, bool invariant = false) {
    if (invariant) return ntri <= 36 ? 4 : 1;
    return launch_split(ntri * Bc);
}
// large launches: four tiles per workgroup (not under ngp_set_batch_invariant: the grouping of a
// thread's partial sums would follow the batch size), and only when every item of the chunk runs on
// the lists kernel: the kernel of the largest trees keeps one tile per workgroup, and a chunk has ONE
// partial-sum layout
inline int contract_tiles_per_wg(const JobGeom &g, int split, long ntri, long Bc, bool has_large_trees) {
    return (!g.invariant && split == 1 && !has_large_trees) ? tiles_per_wg(ntri * Bc) : 1;
}
// Does the series send its stationary trees to the Toeplitz leaf at all?  (Series of up to 256
// points: the general leaf factorises them in one launch, ngp_small_kernels.h — shorter than the
// Toeplitz leaf's chain of sweeps.  Batches beyond what the one-launch path takes, SM_MAX_ITEMS,
// keep the Toeplitz leaf: there it is the faster one — 8,192 stationary items at n = 208: 14.8
// against 21.3 ms; batch-invariant contexts route by the series alone.)
inline bool toep_grad_series(int n, int B, bool option_on, bool short_series, bool invariant) {
    return option_on && n >= TOEP_GRAD_MIN_N && n <= TOEP_GRAD_MAX_N &&
           !(short_series && n <= SM_MAX_NB * NB && (B <= SM_MAX_ITEMS || invariant));
}
// A regular series: a constant non-zero lattice stride over all n points (q: detect_lattice's indices).
inline bool series_regular(const int32_t *q, int n) {
    if (n < 2) return false;
    const long st0 = (long)q[1] - (long)q[0];
    bool regular = st0 != 0;
    for (int i = 2; i < n && regular; ++i) regular = (long)q[i] - (long)q[i - 1] == st0;
    return regular;
}
// parameters of a node, by ngp_op
constexpr int k_nparams[10] = {0, 1, 3, 2, 3, 3, 0, 0, 2, 2};
// k(0) of a tree of Plus, Times and stationary leaves: a leaf's value at distance zero is the
// constant, or the leaf's amplitude (its last parameter)
inline double kernel_k0(const ngp_kernel &k) {
    double st[NGP_MAX_STACK];
    int sp = 0, pi = 0;
    for (int i = 0; i < k.n_ops; ++i) {
        const int op = k.ops[i];
        if (op == NGP_OP_PLUS || op == NGP_OP_TIMES) {
            const double b = st[--sp], a = st[--sp];
            st[sp++] = op == NGP_OP_PLUS ? a + b : a * b;
        } else {
            const int np = k_nparams[op];
            st[sp++] = std::fabs(k.params[pi + np - 1]);
            pi += np;
        }
    }
    return st[0];
}
// Does an item of a regular series (series_regular, on a series toep_grad_series admits) take the
// Toeplitz leaf?  A tree without Linear or ChangePoint nodes, of at most TOEP_LEAF_MAX_OPS operators.
// And: the Gohberg-Semencul sums divide by x_0 = (K^-1)_11 and lose about eps cond(K) of their
// digits; cond(K) <= n k(0) / (noise + jitter).  A matrix whose diagonal shift is below
// TOEP_LEAF_MIN_SHIFT = 1e-9 of its diagonal k(0) (reachable only with a jitter far below the default
// 1e-5: HMC clamps the noise at 1e-12) is not trusted to that formula and takes the general leaf.
// (A checked program, check_program: the evaluator's stack holds it.)
inline bool toep_leaf_item(const ngp_kernel &k, double jitter) {
    if (k.n_ops > TOEP_LEAF_MAX_OPS) return false;
    for (int i = 0; i < k.n_ops; ++i)
        if (k.ops[i] == NGP_OP_LINEAR || k.ops[i] == NGP_OP_CHANGEPOINT) return false;
    return k.noise + jitter >= TOEP_LEAF_MIN_SHIFT * kernel_k0(k);
}
// a batch with items for both leaves (see SPLIT_MIN_ITEMS).  Batch-invariant contexts route by the
// item alone: a stationary tree on a regular series always takes the Toeplitz leaf, whatever travels
// with it
enum GradBatchRoute { GRAD_UNSPLIT, GRAD_PAIR, GRAD_SPLIT };
inline GradBatchRoute grad_batch_route(int B, int n, bool invariant) {
    if (B >= SPLIT_MIN_ITEMS) return GRAD_SPLIT;
    return (invariant || (n >= PAIR_MIN_N && B >= PAIR_MIN_ITEMS)) ? GRAD_PAIR : GRAD_UNSPLIT;
}

// ---- working storage of a gradient leaf's run --------------------------------------------------------
// The blocks a LeafRun asks of the context's workspace, in request order, each once: the request for
// a chunk of Bc items, and what the chunk-size estimate (chunk_for) counts for it per item.  Where the
// two differ the estimate is the smaller one: the halving loop of chunk_for takes up what it leaves
// out, and the chunk sizes (hence the launch grids) of every geometry are pinned to it
// (tests/sanitize/plan_check.cpp restates both).
enum LeafBlockId {
    LEAF_L,       // the padded matrix and its aux rows
    LEAF_DINV,    // block inverses M_j: the Toeplitz path keeps every one for its backward sweep, the general path one
    LEAF_TAB,     // lattice: the tables of the stationary subtrees
    LEAF_SIG,     // lattice: the ChangePoint sigmoids
    LEAF_DTAB,    // lattice: the tables' derivatives
    LEAF_KINV,    // general path: K^-1 [n0 x n0]; Toeplitz path: A = [a' ; x'] (one aux tile)
    LEAF_ALPHA,   // alpha; Toeplitz path: w per distance
    LEAF_QUAD,    // y' K^-1 y
    LEAF_PART,    // partial sums of the contraction
    LEAF_ITEMS,   // the leaf's items sorted by tree size
    LEAF_N_BLOCKS
};
struct LeafBlock {
    bool asked;         // false: never requested (the tables of a job off the lattice)
    size_t bytes;       // the request for a chunk of Bc items
    size_t est_item;    // bytes per item in the chunk-size estimate
};
inline void leaf_run_blocks(const JobGeom &g, bool toep_path, int Bc, LeafBlock (&b)[LEAF_N_BLOCKS]) {
    const size_t GP = NGP_MAX_PARAMS + 1, ntri = (size_t)(g.nb0 * (g.nb0 + 1) / 2), nd = (size_t)((g.n_real + 255) / 256);
    const size_t n0 = (size_t)g.n0, bc = (size_t)Bc, lat = g.lattice ? 1 : 0;
    const size_t tab = lat * 8 * (size_t)g.maxstat * g.R, sig = lat * 8 * (size_t)g.maxcp * g.npts;
    const size_t l = (size_t)g.item_stride * 8, aux = 8 * (size_t)g.naux_pad * n0, blk = 8 * (size_t)NB * NB;
    const size_t kinv = toep_path ? aux : 8 * n0 * n0, part_rows = toep_path ? nd : ntri;
    b[LEAF_L] = {true, l * bc, l};
    // estimate: the general path's single block per item is an omission kept for behaviour's sake
    b[LEAF_DINV] = {true, blk * bc * (toep_path ? (size_t)g.nb0 : 1), toep_path ? blk * g.nb0 : 0};
    b[LEAF_TAB] = {lat != 0, tab * bc, tab};
    b[LEAF_SIG] = {lat != 0, sig * bc, sig};
    b[LEAF_DTAB] = {lat != 0, 3 * tab * bc, 3 * tab};
    b[LEAF_KINV] = {true, kinv * bc, kinv};
    b[LEAF_ALPHA] = {true, 8 * n0 * bc, 8 * n0};
    b[LEAF_QUAD] = {true, 8 * bc, 0};   // estimate: 8 bytes per item, an omission kept for behaviour's sake
    // A chunk of the general path that is cut finer (split 2 or 4) writes at most 4096 partial rows; a
    // coarse one Bc ntri.  Estimate: the coarse figure — the split and the floor depend on Bc, which
    // the estimate is there to choose (kept for behaviour's sake: at most 4096 GP 8 bytes = 3 MB a chunk)
    b[LEAF_PART] = {true,
                    8 * GP * (toep_path ? bc * nd
                                        : std::max<size_t>(bc * ntri * (size_t)grad_contract_split((long)ntri, Bc, g.invariant != 0), 4096)),
                    8 * part_rows * GP};
    b[LEAF_ITEMS] = {true, 4 * (size_t)g.B, 0};   // of the whole leaf, not of a chunk: not an item's cost
}
inline size_t leaf_item_estimate(const JobGeom &g, bool toep_path) {
    LeafBlock b[LEAF_N_BLOCKS];
    leaf_run_blocks(g, toep_path, 1, b);
    size_t n = 0;
    for (const LeafBlock &k : b) n += k.est_item;
    return n;
}

}  // namespace ngp

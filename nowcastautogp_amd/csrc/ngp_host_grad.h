// ngp_host_grad.h — gradient jobs: GradLeaf (a leaf's inputs and results resident on the device),
// GradRoute, grad_leaf_stage / _set_params, LeafRun (working storage, launches, unpack) with chunk_for,
// grad_leaf_run, grad_pair_run (two leaves side by side), the HMC trajectory (grad_leaf_hmc), and
// the public handle ngp_grad_job with grad_stage_impl, ngp_grad_stage, ngp_grad_job_set_params,
// grad_job_run_resident, ngp_grad_job_hmc, ngp_grad_job_info, ngp_grad_job_destroy and
// logml_grad_direct.  The host code behind every HMC step of a fit.
// Included from ngp_api.hip behind that file's own code (check_program, compile_program; PinVec and
// the page-locked pool; ngp_ctx with its workspace and lanes, WsPlan, EventTimer, DevCall, dev_spec;
// FillLists, Lane / lane_of, factor_chunk, ws_layout, stage_up, item_too_large of the staged value
// jobs) and in front of ngp_host_combine.h, which calls GradRoute, grad_stage_impl,
// grad_job_run_resident and logml_grad_direct.  The route rules and the sizes of a run's working
// blocks are ngp_plan.h's.
#pragma once

// ---------------------------------------------------------------------------------------
// gradient jobs: the inputs of ngp_logml_grad_batch kept on the device across calls
// ---------------------------------------------------------------------------------------
// An arena as a table of fields: field k starts at off[k], each rounded up to 256 bytes; off[N]: the end.
template <int N> struct ArenaFields {
    size_t off[N + 1] = {};
    void lay(const size_t (&bytes)[N]) {
        for (int k = 0; k < N; ++k) off[k + 1] = off[k] + ((bytes[k] + 255) & ~(size_t)255);
    }
    size_t end() const { return off[N]; }
};
// everything of a leaf that crosses the bus (the fill lists: FillLists, lattice jobs only)
enum { IO_PROGS, IO_T, IO_Y, IO_Q, IO_FILL_SINGLE, IO_FILL_CHAIN, IO_FILL_OTHER, IO_INFO, IO_LOGDET,
       IO_GRAD, IO_LOGML, IO_FIELDS };
// a leaf's trajectory state: the maps, what goes up, what comes back with its HMC_SC_COUNT per-item
// scalars in the order of their enum; the trace rows stand behind the last field
enum { HMC_SC_U0, HMC_SC_K0, HMC_SC_U1, HMC_SC_K1, HMC_SC_LOGML1, HMC_SC_COUNT };
enum { T_OFF, T_SLOT, T_KIND, T_FROZEN, T_Z, T_PM, T_THETA, T_SCALARS, T_INFO = T_SCALARS + HMC_SC_COUNT, T_FIELDS };

struct GradLeaf {
    bool toep_path = false;                // the Toeplitz gradient path
    ngp_ctx *ctx = nullptr;
    JobGeom g{};
    int B = 0, n = 0;
    PinVec<DevProgram> hp;                 // compiled programs (device parameter order), page-locked: they go up on every run
    std::vector<std::vector<int>> perm;    // device parameter k of item i = the caller's perm[i][k]
    std::vector<int32_t> n_ops, n_params;
    // ONE device arena for everything that crosses the bus:
    //   [programs | t | y | lattice indices | fill lists | info | logdet | gradient | logml]
    unsigned char *io = nullptr;
    ArenaFields<IO_FIELDS> o;
    // lattice jobs: the items by the shape of their reduced program, as in a staged value job
    // (ascending leaf indices; the fill of the main tiles runs on the value jobs' kernels)
    FillLists fill;
    PinVec<unsigned char> h_in, h_out;        // staging copy of a small job's inputs; results
    bool fresh = false;                    // info / logdet still hold the zeros they were staged with
    bool progs_dirty = false;              // set_params since the last upload
    ngp_spec spec{};
    int last_chunk = 0;                    // items per memory-driven chunk of the last run (ngp_grad_job_info)
    // trajectories (ngp_grad_job_hmc): the leaf's latents in the caller's order, on the device from
    // the first trajectory to the job's end
    //   [off | slot || kind | frozen | z | pm || theta | U0 K0 U1 K1 logml1 | info1 || trace rows]
    // kind .. pm go up in one copy per call, z .. info1 come back in one
    unsigned char *hmc = nullptr;
    ArenaFields<T_FIELDS> tj;
    size_t t_rows = 0;                     // trace rows the arena has room for, behind tj.end()
    size_t t_scalar(int k) const { return tj.off[T_SCALARS + k]; }   // k: HMC_SC_U0 ..
    std::vector<int32_t> loff;             // [B + 1] first latent of every item
    PinVec<unsigned char> t_up, t_down;
    // The one place the outcome of a run or a trajectory reaches the leaf, after its scope has
    // synchronised: the staging copy has left h_in, and after a failure the device holds neither the
    // host's programs nor clean info / logdet — the next run sends and clears them.
    void run_ended(ngp_status st) {
        if (!h_in.empty()) PinVec<unsigned char>().swap(h_in);
        if (st) {
            progs_dirty = true;
            fresh = false;
        }
    }
};

// What a gradient evaluation is staged under: the context's spec and the switches that pick its
// routes.  A job keeps the one it was staged with; a combined group of gradient requests is staged
// under its members' common one, which need not be the context's current one (ngp_grad_job_run).
struct GradRoute {
    ngp_spec spec{};
    bool toeplitz = true, invariant = false, short_series = true;
};

static GradRoute grad_route_of(ngp_ctx *c) {   // c->mu held by the caller
    GradRoute r;
    r.spec = c->spec;
    r.toeplitz = c->toeplitz;
    r.invariant = c->invariant;
    r.short_series = c->short_series;
    return r;
}

static bool grad_route_same(const GradRoute &a, const GradRoute &b) {
    const ngp_spec &x = a.spec, &y = b.spec;
    return x.se_form == y.se_form && x.periodic_form == y.periodic_form && x.cp_form == y.cp_form &&
           x.precision == y.precision && x.jitter == y.jitter && x.mixed_tau == y.mixed_tau &&
           x.refine_tol == y.refine_tol && x.refine_max == y.refine_max && a.toeplitz == b.toeplitz &&
           a.invariant == b.invariant && a.short_series == b.short_series;
}

namespace {

void grad_leaf_destroy(GradLeaf *j);

// toep_path: the items are stationary trees on a regular series — aux rows [y' ; e_1'] instead of
// [I ; y'] (the caller, ngp_grad_stage, has checked both)
// yrows: item b's observations are yrows[b][0..n) (y / ldy are then not read) — a subset of a
// caller's batch, or the rows of several callers' arrays in a combined call
ngp_status grad_leaf_stage(ngp_ctx *c, int32_t B, const ngp_kernel *kernels, int32_t n,
                           const double *t, const double *y, int64_t ldy, bool toep_path,
                           GradLeaf **out, const double *const *yrows, const GradRoute &route) {
    if (!c || !out || !kernels || !t || (!y && !yrows) || B <= 0 || n <= 0) return NGP_ERR_ARG;
    *out = nullptr;
    GradLeaf *j = new (std::nothrow) GradLeaf();
    if (!j) return NGP_ERR_TOO_LARGE;
    j->ctx = c;
    // (the leaf before the scope: on a failure the scope ends, synchronised, before the leaf is destroyed)
    std::unique_ptr<GradLeaf, void (*)(GradLeaf *)> guard(j, grad_leaf_destroy);
    j->toep_path = toep_path;
    j->B = B;
    j->n = n;
    j->hp.resize((size_t)B);
    j->perm.resize((size_t)B);
    j->n_ops.resize((size_t)B);
    j->n_params.resize((size_t)B);
    int maxstat = 0, maxcp = 0, maxops = 0, maxtab = 0;
    for (int i = 0; i < B; ++i) {
        int ns = 0, nc = 0, nt = 0;
        ngp_status st = compile_program(&kernels[i], &j->hp[(size_t)i], &j->perm[(size_t)i], &ns, &nc, &nt);
        if (st) return st;
        maxstat = std::max(maxstat, ns);
        maxtab = std::max(maxtab, nt);
        maxcp = std::max(maxcp, nc);
        maxops = std::max(maxops, (int)kernels[i].n_ops);
        j->n_ops[(size_t)i] = kernels[i].n_ops;
        j->n_params[(size_t)i] = kernels[i].n_params;
    }
    // Geometry: the matrix is padded to a multiple of 64 with identity rows/cols (log 1 = 0, a
    // zero in y), and the aux block is [I ; y'] so that the factorisation leaves W = [L^-T ; z'].
    JobGeom &g = j->g;
    g.B = B;
    g.n0 = (n + NB - 1) / NB * NB;
    g.nb0 = g.n0 / NB;
    g.n_real = n;
    g.aux_identity = toep_path ? 0 : 1;
    g.aux_e1 = toep_path ? 1 : 0;
    g.maxops = maxops;
    g.naux = toep_path ? 2 : g.n0 + 1;
    g.naux_pad = toep_path ? NB : g.n0 + NB;
    g.D = 1;
    g.y_shared = (ldy == 0 && !yrows) ? 1 : 0;
    g.ld = g.n0;
    g.item_stride = (int64_t)(g.n0 + g.naux_pad) * g.n0;
    if (item_too_large(g.item_stride)) return NGP_ERR_TOO_LARGE;
    g.npts = g.n0;
    g.maxstat = std::max(maxstat, 1);
    g.maxcp = std::max(maxcp, 1);
    std::vector<int32_t> h_q;
    {
        std::vector<double> real(t, t + n);
        double hh = 0.0;
        int R = 0;
        if (detect_lattice(real, &hh, &h_q, &R)) {
            g.lattice = 1;
            g.h = hh;
            g.R = R;
            h_q.resize((size_t)g.n0, 0);
            // the subtree tables of the reduced programs behind the per-leaf tables (tables_kernel),
            // and the items sorted by the kernel that fills their main tiles (launch_fill)
            g.tab_sub = g.maxstat;
            g.maxstat += maxtab;
            j->fill.sort_items(j->hp.data(), B);
        }
    }
    const int ny = g.y_shared ? 1 : B;
    const int GP = NGP_MAX_PARAMS + 1;
    const FillLists &fl = j->fill;   // (empty off the lattice)
    j->o.lay({sizeof(DevProgram) * (size_t)B, 8 * (size_t)g.n0, 8 * (size_t)ny * g.n0,
              g.lattice ? 4 * (size_t)g.n0 : 0, 4 * fl.single.size(), 4 * fl.chain.size(), 4 * fl.other.size(),
              4 * (size_t)B, 8 * (size_t)B, 8 * (size_t)B * GP, 8 * (size_t)B});
    const size_t *const o = j->o.off;
    int fill_field = IO_FILL_SINGLE;   // FillLists asks for its three lists in the table's order
    j->fill.layout([&](size_t) { return o[fill_field++]; });
    j->h_in.assign(o[IO_GRAD], 0);
    j->h_out.resize(j->o.end() - o[IO_INFO]);
    std::memcpy(j->h_in.data(), j->hp.data(), sizeof(DevProgram) * (size_t)B);
    {
        double *ht = (double *)(j->h_in.data() + o[IO_T]), *hy = (double *)(j->h_in.data() + o[IO_Y]);
        for (int i = 0; i < g.n0; ++i) ht[i] = t[std::min(i, n - 1)];
        for (int b = 0; b < ny; ++b)
            std::memcpy(hy + (size_t)b * g.n0, yrows ? yrows[b] : y + (int64_t)b * ldy, 8 * (size_t)n);
        if (g.lattice) std::memcpy(j->h_in.data() + o[IO_Q], h_q.data(), 4 * (size_t)g.n0);
        j->fill.copy_to(j->h_in.data());
    }
    DevCall call(c);
    j->spec = route.spec;
    g.invariant = route.invariant ? 1 : 0;
    g.short_series = route.short_series ? 1 : 0;
    // (gradient jobs store every tile: their tables are per leaf, and on a regular series the
    // stationary trees — the ones structured storage could serve — are on the Toeplitz path)
    if (call.keep(&j->io, j->o.end()).status()) return call.status();   // nothing is queued yet
    // the front part goes up in one copy (info and logdet arrive as the zeros the factorisation
    // expects): a 24-particle call of a fit on a short series is a chain of dependent launches a
    // few microseconds long, and each separate copy or memset was one more of them
    const ngp_status st = stage_up(call, c->stream, j->io, j->h_in, j->h_in.size());
    if (st) return st;
    j->fresh = true;
    *out = guard.release();
    return NGP_OK;
}

ngp_status grad_leaf_set_params(GradLeaf *j, const double *params, const double *noise) {
    if (!j || !params || !noise) return NGP_ERR_ARG;
    size_t off = 0;
    for (int i = 0; i < j->B; ++i) {
        DevProgram &P = j->hp[(size_t)i];
        const int np = j->n_params[(size_t)i];
        // values are taken as ngp_logml_grad_batch takes them: a parameter the kernels cannot use
        // shows in the item's info, not here
        for (int q = 0; q < np; ++q) P.params[q] = params[off + (size_t)j->perm[(size_t)i][(size_t)q]];
        P.noise = noise[i];
        off += (size_t)np;
    }
    j->progs_dirty = true;
    return NGP_OK;
}

// One evaluation of a leaf in three steps, so that two leaves of a small batch can be in flight side
// by side (grad_pair_run): lay the working storage out in the context's workspace, enqueue
// everything on a lane's streams (upload of new parameters ... results on their way back), and,
// after the lane has been synchronised, unpack.
struct LeafRun {
    GradLeaf *j = nullptr;
    int Bc = 0;
    void *d[LEAF_N_BLOCKS] = {};    // the working blocks of a chunk of Bc items: LeafBlockId, ngp_plan.h
    std::vector<int32_t> h_items;   // read by a queued copy: a LeafRun is declared before its run's scope
    bool items_ready = false;       // a later evaluation of a trajectory: d[LEAF_ITEMS] holds the sorted items
    double *splitk = nullptr;       // pair runs: the context's split-k buffer for this leaf's value kernels

    // the blocks requested from `dalloc` (measured, then taken), in the list's order
    ngp_status layout(WsPlan &dalloc) {
        LeafBlock b[LEAF_N_BLOCKS];
        leaf_run_blocks(j->g, j->toep_path, Bc, b);
        for (int k = 0; k < LEAF_N_BLOCKS; ++k)
            if (b[k].asked)
                if (const ngp_status r = dalloc(&d[k], b[k].bytes)) return r;
        return NGP_OK;
    }

    // everything of the evaluation on the lane's streams, as steps of the run's scope, which waits for
    // the lane; tm: the scope's timer of that lane
    // copy_out: the results follow the last kernel into h_out (a trajectory reads them on the device)
    void launch(DevCall &call, const Lane &ln, EventTimer &tm, bool no_lane_split, bool copy_out = true) {
        ngp_ctx *c = j->ctx;
        const JobGeom &g = j->g;
        const int B = j->B;
        const bool tp = j->toep_path;
        const int GP = NGP_MAX_PARAMS + 1;
        hipStream_t s = ln.main;
        const DevSpec sp = dev_spec(j->spec);
        if (!items_ready) h_items.assign((size_t)B, 0);
        unsigned char *const io = j->io;
        const size_t *const o = j->o.off;
        void *const d_prog = io, *const d_t = io + o[IO_T], *const d_y = io + o[IO_Y],
                    *const d_q = g.lattice ? io + o[IO_Q] : nullptr, *const d_info = io + o[IO_INFO],
                    *const d_logdet = io + o[IO_LOGDET], *const d_grad = io + o[IO_GRAD],
                    *const d_logml = io + o[IO_LOGML];
        // new parameters for the same trees: the programs go up again, nothing else.  On a lattice the
        // first kernel of the chain (tables_kernel) fetches them from the page-locked host copy itself
        // and leaves the device copy for the rest — a copy ahead of the chain cost 20 us of a 24-item
        // call's 110.
        const bool fetch_in_kernel = j->progs_dirty && g.lattice && g.n0 > 0 &&
                                     pinned_pool().is_pinned(j->hp.data());
        if (j->progs_dirty && !fetch_in_kernel) call.up(d_prog, j->hp.data(), sizeof(DevProgram) * (size_t)B, s);
        // a re-run: info | logdet are contiguous in the arena (short jobs: written outright)
        if (!j->fresh && !small_job(g, Bc)) call.zero(d_info, o[IO_GRAD] - o[IO_INFO], s);
        // (for the evaluations that follow in this scope; a failure takes both back: GradLeaf::run_ended)
        j->progs_dirty = false;
        j->fresh = false;
        for (int b0 = 0; b0 < B; b0 += Bc) {
            const int bc = std::min(Bc, B - b0);
            ChunkPtrs p{};
            p.L = (double *)d[LEAF_L];
            p.dinv = (double *)d[LEAF_DINV];
            p.progs = (const DevProgram *)d_prog + b0;
            p.progs_src = fetch_in_kernel ? j->hp.data() + b0 : nullptr;
            p.t0 = (const double *)d_t;
            p.taux = (const double *)d_t;
            p.y0 = (const double *)d_y + (g.y_shared ? 0 : (int64_t)b0 * g.n0);
            p.logdet = (double *)d_logdet + b0;
            p.info = (int32_t *)d_info + b0;
            p.tab = (double *)d[LEAF_TAB];
            p.sig = (double *)d[LEAF_SIG];
            p.qpts = (const int32_t *)d_q;
            p.dtab = (double *)d[LEAF_DTAB];
            p.splitk_part = splitk;
            if (g.lattice) j->fill.share_of(io, b0, bc, &p);
            if (g.lattice) call.timed(tm, 4, 0.0, 0.0, [&] { launch_tables(g, p, bc, sp, s); });
            call.timed(tm, cost_fill_grad(g, bc, tp), [&] { launch_fill(g, p, bc, sp, s); });
            const size_t mstep = tp ? (size_t)bc * NB * NB : 0;
            call.run([&] { factor_chunk(ln, g, p, bc, tm, mstep, nullptr, nullptr, nullptr, no_lane_split); });
            if (tp) {
                // z'z, then A = X K^-1 by one backward sweep of the two aux rows
                call.timed(tm, cost_toep_quad(g, bc),
                       [&] { launch_toep_quad(g, (const double *)d[LEAF_L], (double *)d[LEAF_QUAD], bc, s); });
                for (int cc = g.nb0 - 1; cc >= 0; --cc)
                    call.timed(tm, cost_toep_back(bc, cc), [&] {
                        launch_aux_back(g, p, p.dinv, mstep, (double *)d[LEAF_KINV], 0, bc, cc, s);
                    });
            } else {
                const bool kinv_small = kinv_route(g, bc) == KINV_SMALL;
                call.timed(tm, cost_kinv(g, bc), [&] {
                    if (kinv_small)
                        launch_grad_kinv_small(g, (const double *)d[LEAF_L], (double *)d[LEAF_KINV], (double *)d[LEAF_ALPHA],
                                               (double *)d[LEAF_QUAD], bc, s);
                    else
                        launch_grad_kinv(g, (const double *)d[LEAF_L], (double *)d[LEAF_KINV], (double *)d[LEAF_ALPHA],
                                         (double *)d[LEAF_QUAD], bc, s, ln.side, ln.fork, ln.join);
                });
            }
            // the chunk's items sorted by tree size: every size class runs on the contraction kernel
            // sized for it
            const bool by_size = contract_by_size(g, tp, bc);
            int32_t counts[GRAD_BUCKETS] = {};
            if (by_size) for (int i = 0; i < bc; ++i) ++counts[grad_bucket(j->n_ops[(size_t)(b0 + i)])];
            if (by_size && !items_ready) {
                int32_t pos[GRAD_BUCKETS], acc = 0;
                for (int k = 0; k < GRAD_BUCKETS; ++k) { pos[k] = acc; acc += counts[k]; }
                for (int i = 0; i < bc; ++i)
                    h_items[(size_t)b0 + (size_t)pos[grad_bucket(j->n_ops[(size_t)(b0 + i)])]++] = i;
                call.up((int32_t *)d[LEAF_ITEMS] + b0, h_items.data() + b0, 4 * (size_t)bc, s);
            }
            if (tp) {
                call.timed(tm, cost_toep_grad(g, bc), [&] {
                    launch_toep_grad(g, p, (const double *)d[LEAF_KINV], (double *)d[LEAF_ALPHA],
                                     (const double *)d[LEAF_QUAD], (double *)d[LEAF_PART],
                                     (double *)d_grad + (int64_t)b0 * GP, (double *)d_logml + b0, bc, sp,
                                     s, by_size ? (const int32_t *)d[LEAF_ITEMS] + b0 : nullptr, counts);
                });
            } else {
                call.timed(tm, cost_contract(g, bc), [&] {
                    launch_grad_contract(g, p, (const double *)d[LEAF_KINV], (const double *)d[LEAF_ALPHA],
                                         (const double *)d[LEAF_QUAD], (double *)d[LEAF_PART],
                                         (double *)d_grad + (int64_t)b0 * GP, (double *)d_logml + b0,
                                         bc, sp, s, by_size ? (const int32_t *)d[LEAF_ITEMS] + b0 : nullptr,
                                         counts, ln.side, ln.fork, ln.join);
                });
            }
        }
        if (copy_out) call.down(j->h_out.data(), d_info, j->h_out.size(), s);
    }

    // after the lane is synchronised: device parameter order -> caller's order; d/d noise last
    void unpack(double *logml, double *grad, int32_t *info) {
        const int GP = NGP_MAX_PARAMS + 1;
        const int32_t *h_info = (const int32_t *)j->h_out.data();
        const size_t *const o = j->o.off;
        const double *h_grad = (const double *)(j->h_out.data() + (o[IO_GRAD] - o[IO_INFO])),
                     *h_lm = (const double *)(j->h_out.data() + (o[IO_LOGML] - o[IO_INFO]));
        size_t off = 0;
        for (int i = 0; i < j->B; ++i) {
            const int np = j->n_params[(size_t)i];
            for (int k = 0; k < np; ++k)
                grad[off + (size_t)j->perm[(size_t)i][(size_t)k]] = h_grad[(size_t)i * GP + (size_t)k];
            grad[off + (size_t)np] = h_grad[(size_t)i * GP + (size_t)np];
            off += (size_t)np + 1;
            if (logml) logml[i] = h_lm[(size_t)i];
            if (info) info[i] = h_info[(size_t)i];
        }
    }
};

// The memory-driven chunk of a leaf's run, laid out in the context's workspace (r.Bc and the d_*
// pointers): as many items as the memory figure allows, halved when the device cannot hold that
// after all (other handles, rounding).
ngp_status chunk_for(ngp_ctx *c, LeafRun &r) {
    const size_t B = (size_t)r.j->B, item_bytes = leaf_item_estimate(r.j->g, r.j->toep_path);
    if (B * item_bytes > c->mem_cap) c->refresh_mem_cap();   // large job: today's figure
    r.Bc = (int)std::min<size_t>(std::min<size_t>(B, MAX_CHUNK_ITEMS), std::max<size_t>(1, c->mem_cap / item_bytes));
    for (;; r.Bc = (r.Bc + 1) / 2) {
        const ngp_status st = ws_layout(c, [&](WsPlan &w) { return r.layout(w); });
        if (!st) r.j->last_chunk = r.Bc;
        if (st != NGP_ERR_TOO_LARGE || r.Bc <= 1) return st;
    }
}

ngp_status grad_leaf_run(GradLeaf *j, double *logml, double *grad, int32_t *info) {
    if (!j || !grad) return NGP_ERR_ARG;
    ngp_ctx *c = j->ctx;
    LeafRun r;
    r.j = j;
    DevCall call(c);
    if (call.status()) return call.status();
    const ngp_status fit = chunk_for(c, r);
    if (fit) return fit;   // nothing is queued yet
    r.launch(call, lane_of(c), call.tm, false);
    const ngp_status st = call.sync();
    j->run_ended(st);
    if (!st) r.unpack(logml, grad, info);
    return st;
}

// The two leaves of a SMALL mixed batch side by side, each on its own pair of streams (the lanes of
// the two-lane sweep): one after the other they are two chains of dependent launches where the
// unsplit batch is one (64 items at n = 2048: 16.3 ms against 15.3).  Both as single chunks in one
// workspace reservation; NGP_ERR_TOO_LARGE if that does not fit (the caller then runs them in turn).
ngp_status grad_pair_run(GradLeaf *a, double *lm_a, double *g_a, int32_t *info_a, GradLeaf *b,
                         double *lm_b, double *g_b, int32_t *info_b) {
    ngp_ctx *c = a->ctx;
    LeafRun ra, rb;
    ra.j = a;
    rb.j = b;
    DevCall call(c);
    if (call.status()) return call.status();
    if (!c->make_lanes(2)) return NGP_ERR_TOO_LARGE;
    ra.Bc = a->last_chunk = a->B;
    rb.Bc = b->last_chunk = b->B;
    WsPlan measure{c, true}, take{c, false};
    (void)ra.layout(measure);
    (void)rb.layout(measure);
    if (measure.total > c->mem_cap) c->refresh_mem_cap();
    if (measure.total > c->mem_cap) return NGP_ERR_TOO_LARGE;
    ngp_status st = c->ws_reserve(measure.total);
    if (st) return st;
    if ((st = ra.layout(take)) || (st = rb.layout(take))) return st;   // nothing is queued yet
    // the Toeplitz leaf runs on the value kernels: their split-k fat steps of late columns (small
    // chunks) need the context's buffer, which factor_chunk only reserves for a chunk it owns whole
    if (b->toep_path && splitk_eligible(b->g, b->B, false, false) && c->splitk_reserve(b->B) == NGP_OK)
        rb.splitk = c->splitk_part;
    const Lane l0 = lane_of(c);
    const Lane l1 = lane_of(c, 1);
    EventTimer &tm1 = call.second_lane();
    // what the context's stream holds (the staging copies of both leaves) comes first on lane 1 too
    call.run([&] {
        (void)hipEventRecord(c->ev_lane_go, c->stream);
        (void)hipStreamWaitEvent(l1.main, c->ev_lane_go, 0);
    });
    ra.launch(call, l0, call.tm, true);
    rb.launch(call, l1, tm1, true);
    st = call.sync();
    a->run_ended(st);
    b->run_ended(st);
    if (st) return st;
    ra.unpack(lm_a, g_a, info_a);
    rb.unpack(lm_b, g_b, info_b);
    return NGP_OK;
}

// One trajectory of a leaf (ngp_grad_job_hmc): kind / frozen / z0 / mom and the outputs are the
// leaf's latents back to back in the caller's order.  The working storage is laid out once, the
// n_leapfrog + 1 evaluations are LeafRun::launch as ngp_grad_job_run enqueues it, the step kernel
// between them writes the next parameters into the device programs; one copy back, one
// synchronisation.  z_trace: null or [n_leapfrog + 1][latents of the leaf].
struct HmcOut {
    double *z1, *mom1, *theta1, *U0, *K0, *U1, *K1, *lm1;
    int32_t *info1;
    double *trace;
};

ngp_status grad_leaf_hmc(GradLeaf *j, const ngp_hmc_config *cfg, const uint8_t *kind,
                         const uint8_t *frozen, const double *z0, const double *mom, const HmcOut &o) {
    ngp_ctx *c = j->ctx;
    const int B = j->B, L = cfg->n_leapfrog;
    // read by queued copies: before the scope
    PinVec<unsigned char> maps;
    LeafRun r;
    r.j = j;
    DevCall call(c);
    if (call.status()) return call.status();
    const size_t *const t = j->tj.off;   // (the table is the leaf's: laid out below, at the first trajectory)
    const size_t rows = o.trace ? (size_t)L + 1 : 0;
    if (!j->hmc || rows > j->t_rows) {
        // first trajectory of the job (or the first that asks for a longer trace): the arena, and
        // the maps that do not change — item offsets, and the inverse of GradLeaf::perm
        j->loff.assign((size_t)B + 1, 0);
        for (int i = 0; i < B; ++i) j->loff[(size_t)i + 1] = j->loff[(size_t)i] + j->n_params[(size_t)i] + 1;
        const size_t NL = (size_t)j->loff[(size_t)B];
        const size_t sc = 8 * (size_t)B;
        j->tj.lay({4 * ((size_t)B + 1), NL, NL, NL, 8 * NL, 8 * NL, 8 * NL, sc, sc, sc, sc, sc, 4 * (size_t)B});
        unsigned char *q = nullptr;
        if (call.keep(&q, j->tj.end() + 8 * NL * rows).status()) return call.status();   // nothing is queued yet
        c->release(j->hmc);
        j->hmc = q;
        j->t_rows = rows;
        j->t_up.assign(t[T_THETA] - t[T_KIND], 0);
        j->t_down.assign(j->tj.end() - t[T_Z], 0);
        maps.assign(t[T_KIND], 0);
        std::memcpy(maps.data(), j->loff.data(), 4 * ((size_t)B + 1));
        for (int i = 0; i < B; ++i) {
            unsigned char *sl = maps.data() + t[T_SLOT] + j->loff[(size_t)i];
            const int np = j->n_params[(size_t)i];
            for (int k = 0; k < np; ++k) sl[j->perm[(size_t)i][(size_t)k]] = (unsigned char)k;
            sl[np] = (unsigned char)np;
        }
        // the arena is the job's only with its maps in it: a round trip of its own, once per job
        if (call.up(j->hmc, maps.data(), maps.size()).wait()) {
            c->release(j->hmc);
            j->hmc = nullptr;
            j->t_rows = 0;
            return call.status();   // synchronised
        }
    }
    const size_t NL = (size_t)j->loff[(size_t)B];
    {
        unsigned char *up = j->t_up.data();
        std::memcpy(up, kind, NL);
        if (frozen) std::memcpy(up + (t[T_FROZEN] - t[T_KIND]), frozen, NL);
        else std::memset(up + (t[T_FROZEN] - t[T_KIND]), 0, NL);
        std::memcpy(up + (t[T_Z] - t[T_KIND]), z0, 8 * NL);
        std::memcpy(up + (t[T_PM] - t[T_KIND]), mom, 8 * NL);
    }
    const ngp_status fit = chunk_for(c, r);
    if (fit) return fit;   // nothing is queued
    hipStream_t s = c->stream;
    unsigned char *const h = j->hmc;
    HmcDev a{};
    a.progs = (DevProgram *)j->io;
    a.grad = (const double *)(j->io + j->o.off[IO_GRAD]);
    a.logml = (const double *)(j->io + j->o.off[IO_LOGML]);
    a.info = (const int32_t *)(j->io + j->o.off[IO_INFO]);
    a.off = (const int32_t *)(h + t[T_OFF]);
    a.slot = h + t[T_SLOT];
    a.kind = h + t[T_KIND];
    a.frozen = h + t[T_FROZEN];
    a.z = (double *)(h + t[T_Z]);
    a.pm = (double *)(h + t[T_PM]);
    a.theta = (double *)(h + t[T_THETA]);
    // the per-item scalars, by HMC_SC_*: where the device writes them, where the caller wants them
    double **const dev_sc[HMC_SC_COUNT] = {&a.U0, &a.K0, &a.U1, &a.K1, &a.lm1};
    double *const host_sc[HMC_SC_COUNT] = {o.U0, o.K0, o.U1, o.K1, o.lm1};
    for (int k = 0; k < HMC_SC_COUNT; ++k) *dev_sc[k] = (double *)(h + j->t_scalar(k));
    a.info1 = (int32_t *)(h + t[T_INFO]);
    a.eps = cfg->eps;
    for (int k = 0; k < 5; ++k) {
        a.mu[k] = k >= 2 ? cfg->prior_mu[k] : 0.0;
        a.sigma[k] = k >= 2 ? cfg->prior_sigma[k] : 1.0;
    }
    a.B = B;
    double *const trace = o.trace ? (double *)(h + j->tj.end()) : nullptr;
    // the device writes its own parameters from here on: whatever set_params left is superseded
    j->progs_dirty = false;
    call.up(h + t[T_KIND], j->t_up.data(), j->t_up.size());
    auto step = [&](int phase, int row) {
        a.phase = phase;
        a.trace = trace && row >= 0 ? trace + (size_t)row * NL : nullptr;
        call.timed(call.tm, 4, 0.0, 0.0, [&] { launch_hmc_step(a, s); });
    };
    step(HMC_INIT, 0);
    for (int ev = 0; ev <= L && !call.status(); ++ev) {
        r.launch(call, lane_of(c), call.tm, false, false);
        r.items_ready = true;
        step(ev == L ? HMC_LAST : ev == 0 ? HMC_FIRST : HMC_MIDDLE, ev == L ? -1 : ev + 1);
    }
    call.down(j->t_down.data(), h + t[T_Z], j->t_down.size());
    if (trace) call.down(o.trace, trace, 8 * NL * ((size_t)L + 1));
    const ngp_status st = call.sync();
    j->run_ended(st);   // (after a failure the device programs are not the host's: the next run sends them)
    if (st) return st;
    const unsigned char *dn = j->t_down.data();
    auto at = [&](size_t t_x) { return dn + (t_x - t[T_Z]); };
    std::memcpy(o.z1, at(t[T_Z]), 8 * NL);
    std::memcpy(o.mom1, at(t[T_PM]), 8 * NL);
    std::memcpy(o.theta1, at(t[T_THETA]), 8 * NL);
    for (int k = 0; k < HMC_SC_COUNT; ++k) std::memcpy(host_sc[k], at(j->t_scalar(k)), 8 * (size_t)B);
    std::memcpy(o.info1, at(t[T_INFO]), 4 * (size_t)B);
    // the host copy of the programs follows the device's: the parameters of the last evaluation
    for (int i = 0; i < B; ++i) {
        DevProgram &P = j->hp[(size_t)i];
        const double *th = o.theta1 + j->loff[(size_t)i];
        const int np = j->n_params[(size_t)i];
        for (int q = 0; q < np; ++q) P.params[q] = th[j->perm[(size_t)i][(size_t)q]];
        P.noise = th[np];
    }
    return NGP_OK;
}

void grad_leaf_destroy(GradLeaf *j) {
    if (!j) return;
    {
        DevCall call(j->ctx);
        // a staging buffer that was kept must outlive its copy
        if (!j->h_in.empty()) call.pending();
        (void)call.sync();
        j->ctx->release(j->io);
        j->ctx->release(j->hmc);
    }
    delete j;
}

}  // namespace

// A leaf's share of the caller's batch: the caller's items it carries (idx, ascending) and the job's
// offsets of an item's parameters (poff) and of its latents / gradient entries (goff).  A leaf that
// carries the whole batch takes the caller's arrays as they are; otherwise its inputs are gathered
// into the leaf's order and its outputs scattered back, array by array.
struct LeafShare {
    GradLeaf *leaf;
    const std::vector<int32_t> &idx;
    const std::vector<size_t> &goff, &poff;     // [B + 1]
    bool whole() const { return idx.size() + 1 == goff.size(); }
    size_t items() const { return idx.size(); }
    // entries of the share in an array laid out by `off` (goff or poff)
    size_t count(const std::vector<size_t> &off) const {
        size_t n = 0;
        for (int32_t i : idx) n += off[(size_t)i + 1] - off[(size_t)i];
        return n;
    }
    // arrays with a run of entries per item
    template <class T> void gather(const std::vector<size_t> &off, const T *all, T *mine) const {
        for (int32_t i : idx) mine = std::copy(all + off[(size_t)i], all + off[(size_t)i + 1], mine);
    }
    template <class T> void scatter(const std::vector<size_t> &off, const T *mine, T *all) const {
        for (int32_t i : idx) {
            const size_t len = off[(size_t)i + 1] - off[(size_t)i];
            std::copy(mine, mine + len, all + off[(size_t)i]);
            mine += len;
        }
    }
    // arrays with one entry per item (all: may be null, an output the caller does not want)
    template <class T> void gather_items(const T *all, T *mine) const {
        for (size_t a = 0; a < idx.size(); ++a) mine[a] = all[idx[a]];
    }
    template <class T> void scatter_items(const T *mine, T *all) const {
        for (size_t a = 0; all && a < idx.size(); ++a) all[idx[a]] = mine[a];
    }
};

// The public handle: the batch as the caller sees it, carried by up to two leaves — the items that
// are stationary trees, when the series is regular, on the Toeplitz path, the others on the general
// one — with the index maps that scatter results and parameters.
struct ngp_grad_job {
    ngp_ctx *ctx = nullptr;
    int B = 0;
    GradLeaf *gen = nullptr, *toep = nullptr;
    std::vector<int32_t> idx_gen, idx_toep;     // leaf item -> caller's item
    std::vector<size_t> poff, goff;             // [B + 1] offsets of an item's parameters / gradient
    // the leaves in the order they run — general, then Toeplitz — each with its share of the batch
    LeafShare share(int k) const { return LeafShare{k ? toep : gen, k ? idx_toep : idx_gen, goff, poff}; }
    // a leaf of some of the items, per leaf: its parameters and noises, or its gradient and logml,
    // in the leaf's order; its info
    std::vector<double> buf[2];
    std::vector<int32_t> buf_info[2];
    bool side_by_side = false;                  // a small split batch: both leaves in flight together
    // Small jobs keep a host copy of what a ONE-SHOT call over their items would take (trees and
    // current parameters in the caller's order, dates, observation rows): when several tasks run
    // their jobs at the same moment — the leapfrog steps of the per-scenario HMC moves of
    // forecast_with_nowcasts, src/forecasting.jl:145-148 — the runs are combined into one call
    // over all their items ("combining" section); alone, a run uses the resident inputs as before.
    std::vector<int32_t> h_ops;
    std::vector<double> h_params, h_t, h_y;
    std::vector<ngp_kernel> h_k;
    int32_t n = 0;
    int64_t h_ldy = 0;
    GradRoute route;                            // what the job was staged under
    // The one-shot form of the job follows the resident one (a combined run reads it): item i's
    // parameters are p[off[i] ..], its noise is noise[i], or stands behind its parameters (null)
    void host_copy_follows(const double *p, const std::vector<size_t> &off, const double *noise) {
        if (h_k.empty()) return;
        for (size_t i = 0; i < (size_t)B; ++i) {
            const size_t np = poff[i + 1] - poff[i];
            std::copy(p + off[i], p + off[i] + np, h_params.data() + poff[i]);
            h_k[i].noise = noise ? noise[i] : p[off[i] + np];
        }
    }
};
// host copies up to this size (64 particles x 2,049 points = 1 MB; a lockstep job of 12,800 items
// is 210 MB and has no use for company)
static constexpr size_t GRAD_JOB_HOST_COPY_BYTES = (size_t)16 << 20;

static ngp_status grad_stage_impl(ngp_ctx *c, int32_t B, const ngp_kernel *kernels, int32_t n,
                                  const double *t, const double *y, int64_t ldy,
                                  const double *const *yrows, ngp_grad_job **out,
                                  bool keep_host = false, const GradRoute *route_in = nullptr) {
    if (!c || !out || !kernels || !t || (!y && !yrows) || B <= 0 || n <= 0) return NGP_ERR_ARG;
    *out = nullptr;
    for (int i = 0; i < B; ++i) {
        ngp_status st = check_program(&kernels[i]);
        if (st) return st;
    }
    std::unique_ptr<ngp_grad_job> j(new (std::nothrow) ngp_grad_job());
    if (!j) return NGP_ERR_TOO_LARGE;
    j->ctx = c;
    j->B = B;
    j->poff.assign((size_t)B + 1, 0);
    j->goff.assign((size_t)B + 1, 0);
    for (int i = 0; i < B; ++i) {
        j->poff[(size_t)i + 1] = j->poff[(size_t)i] + (size_t)kernels[i].n_params;
        j->goff[(size_t)i + 1] = j->goff[(size_t)i] + (size_t)kernels[i].n_params + 1;
    }
    GradRoute route;
    if (route_in) {
        route = *route_in;
    } else {
        std::lock_guard<std::mutex> lk(c->mu);
        route = grad_route_of(c);
    }
    // the Toeplitz leaf: which series, which of their items — ngp_plan.h
    bool regular = false;
    if (toep_grad_series(n, B, route.toeplitz, route.short_series, route.invariant)) {
        std::vector<double> real(t, t + n);
        std::vector<int32_t> q;
        double hh = 0.0;
        int R = 0;
        regular = detect_lattice(real, &hh, &q, &R) && series_regular(q.data(), n);
    }
    for (int i = 0; i < B; ++i)
        (regular && toep_leaf_item(kernels[i], route.spec.jitter) ? j->idx_toep : j->idx_gen).push_back(i);
    // a mixed batch: both leaves in turn, side by side, or everything on the general leaf
    if (!j->idx_gen.empty() && !j->idx_toep.empty()) {
        const GradBatchRoute br = grad_batch_route(B, n, route.invariant);
        if (br == GRAD_PAIR) {
            j->side_by_side = true;
        } else if (br == GRAD_UNSPLIT) {
            j->idx_toep.clear();
            j->idx_gen.resize((size_t)B);
            for (int i = 0; i < B; ++i) j->idx_gen[(size_t)i] = i;
        }
    }
    auto stage_leaf = [&](const LeafShare &sh, bool toep_path, GradLeaf **leaf) -> ngp_status {
        if (!sh.items()) return NGP_OK;
        if (sh.whole()) return grad_leaf_stage(c, B, kernels, n, t, y, ldy, toep_path, leaf, yrows, route);
        const int32_t nb = (int32_t)sh.items();
        std::vector<ngp_kernel> ks(sh.items());
        sh.gather_items(kernels, ks.data());
        if (!yrows && ldy == 0)
            return grad_leaf_stage(c, nb, ks.data(), n, t, y, 0, toep_path, leaf, nullptr, route);
        std::vector<const double *> rows(sh.items());   // the leaf's rows where they lie
        if (yrows) sh.gather_items(yrows, rows.data());
        else for (size_t a = 0; a < sh.items(); ++a) rows[a] = y + (int64_t)sh.idx[a] * ldy;
        return grad_leaf_stage(c, nb, ks.data(), n, t, nullptr, 0, toep_path, leaf, rows.data(), route);
    };
    ngp_status st = stage_leaf(j->share(0), false, &j->gen);
    if (!st) st = stage_leaf(j->share(1), true, &j->toep);
    if (st) {
        grad_leaf_destroy(j->gen);
        grad_leaf_destroy(j->toep);
        return st;
    }
    j->n = n;
    j->route = route;
    const bool shared = !yrows && ldy == 0;
    if (keep_host && (size_t)(shared ? 1 : B) * (size_t)n * 8 <= GRAD_JOB_HOST_COPY_BYTES) {
        j->h_t.assign(t, t + n);
        j->h_ldy = shared ? 0 : n;
        j->h_y.resize((size_t)(shared ? 1 : B) * (size_t)n);
        for (int b = 0; b < (shared ? 1 : B); ++b)
            std::memcpy(j->h_y.data() + (size_t)b * n, yrows ? yrows[b] : y + (int64_t)b * ldy, 8 * (size_t)n);
        size_t nops = 0;
        for (int i = 0; i < B; ++i) nops += (size_t)kernels[i].n_ops;
        j->h_ops.reserve(nops);
        j->h_params.resize(std::max<size_t>(j->poff[(size_t)B], 1));
        j->h_k.resize((size_t)B);
        for (int i = 0; i < B; ++i) {
            j->h_ops.insert(j->h_ops.end(), kernels[i].ops, kernels[i].ops + kernels[i].n_ops);
            if (kernels[i].n_params > 0)
                std::memcpy(j->h_params.data() + j->poff[(size_t)i], kernels[i].params,
                            8 * (size_t)kernels[i].n_params);
        }
        size_t o = 0;
        for (int i = 0; i < B; ++i) {
            j->h_k[(size_t)i] = ngp_kernel{kernels[i].n_ops, kernels[i].n_params, j->h_ops.data() + o,
                                           j->h_params.data() + j->poff[(size_t)i], kernels[i].noise};
            o += (size_t)kernels[i].n_ops;
        }
    }
    *out = j.release();
    return NGP_OK;
}

extern "C" ngp_status ngp_grad_stage(ngp_ctx *c, int32_t B, const ngp_kernel *kernels, int32_t n,
                                     const double *t, const double *y, int64_t ldy,
                                     ngp_grad_job **out) {
    if (!y) return NGP_ERR_ARG;
    return grad_stage_impl(c, B, kernels, n, t, y, ldy, nullptr, out, true);
}

extern "C" ngp_status ngp_grad_job_set_params(ngp_grad_job *j, const double *params,
                                              const double *noise) {
    if (!j || !params || !noise) return NGP_ERR_ARG;
    for (int k = 0; k < 2; ++k) {
        const LeafShare sh = j->share(k);
        if (!sh.leaf) continue;
        ngp_status st;
        if (sh.whole()) {
            st = grad_leaf_set_params(sh.leaf, params, noise);
        } else {
            const size_t np = sh.count(j->poff);
            std::vector<double> &b = j->buf[k];   // [parameters | noises]
            b.resize(np + sh.items());
            sh.gather(j->poff, params, b.data());
            sh.gather_items(noise, b.data() + np);
            st = grad_leaf_set_params(sh.leaf, b.data(), b.data() + np);
        }
        if (st) return st;
    }
    j->host_copy_follows(params, j->poff, noise);
    return NGP_OK;
}

// the run on the job's resident inputs (ngp_grad_job_run, defined in the "combining" section, comes
// here when the job is alone)
static ngp_status grad_job_run_resident(ngp_grad_job *j, double *logml, double *grad, int32_t *info) {
    if (!j || !grad) return NGP_ERR_ARG;
    // where a leaf's results land: in the caller's arrays, or in the job's scratch [gradient | logml], info
    struct Out { double *lm, *g; int32_t *info; } o[2];
    LeafShare sh[2] = {j->share(0), j->share(1)};
    for (int k = 0; k < 2; ++k) {
        o[k] = Out{logml, grad, info};
        if (!sh[k].leaf || sh[k].whole()) continue;
        const size_t ng = sh[k].count(j->goff);
        j->buf[k].resize(ng + sh[k].items());
        j->buf_info[k].resize(sh[k].items());
        o[k] = Out{j->buf[k].data() + ng, j->buf[k].data(), j->buf_info[k].data()};
    }
    auto deliver = [&](int k) {
        if (sh[k].whole()) return;
        sh[k].scatter(j->goff, o[k].g, grad);
        sh[k].scatter_items(o[k].lm, logml);
        sh[k].scatter_items(o[k].info, info);
    };
    if (j->side_by_side && j->gen && j->toep) {
        const ngp_status st = grad_pair_run(j->gen, o[0].lm, o[0].g, o[0].info, j->toep, o[1].lm, o[1].g, o[1].info);
        if (st == NGP_OK) {
            deliver(0);
            deliver(1);
            return NGP_OK;
        }
        if (st != NGP_ERR_TOO_LARGE) return st;   // no room for both at once: one after the other
    }
    for (int k = 0; k < 2; ++k) {
        if (!sh[k].leaf) continue;
        const ngp_status st = grad_leaf_run(sh[k].leaf, o[k].lm, o[k].g, o[k].info);
        if (st) return st;
        deliver(k);
    }
    return NGP_OK;
}

extern "C" ngp_status ngp_grad_job_hmc(ngp_grad_job *j, const void *cfg_, const void *kind_,
                                       const void *frozen_, const double *z0, const double *mom,
                                       double *z1, double *mom1, double *theta1, double *U0, double *K0,
                                       double *U1, double *K1, double *logml1, int32_t *info1,
                                       double *z_trace) {
    const ngp_hmc_config *cfg = (const ngp_hmc_config *)cfg_;
    const uint8_t *kind = (const uint8_t *)kind_, *frozen = (const uint8_t *)frozen_;
    if (!j || !cfg || !kind || !z0 || !mom || !z1 || !mom1 || !theta1 || !U0 || !K0 || !U1 || !K1 ||
        !logml1 || !info1)
        return NGP_ERR_ARG;
    if (cfg->n_leapfrog < 1 || !std::isfinite(cfg->eps)) return NGP_ERR_ARG;
    if (cfg->n_leapfrog > 65536) return NGP_ERR_TOO_LARGE;   // the limit include/ngp.h states
    const size_t NL = j->goff[(size_t)j->B];
    for (size_t q = 0; q < NL; ++q) {
        const int kd = kind[q];
        if (kd > 4) return NGP_ERR_ARG;
        if (kd >= 2 && !(cfg->prior_sigma[kd] > 0.0 && std::isfinite(cfg->prior_sigma[kd]) &&
                         std::isfinite(cfg->prior_mu[kd])))
            return NGP_ERR_ARG;
    }
    const size_t rows = z_trace ? (size_t)cfg->n_leapfrog + 1 : 0;
    // items are independent: the whole trajectory of the general leaf, then that of the Toeplitz leaf
    // (each under the context's lock; a failure of the second leaves the job as include/ngp.h says)
    for (int k = 0; k < 2; ++k) {
        const LeafShare sh = j->share(k);
        if (!sh.leaf) continue;
        if (sh.whole()) {
            const ngp_status st = grad_leaf_hmc(sh.leaf, cfg, kind, frozen, z0, mom,
                                                HmcOut{z1, mom1, theta1, U0, K0, U1, K1, logml1, info1, z_trace});
            if (st) return st;
            continue;
        }
        // a leaf of some of the items: their latents gathered, the outputs scattered back
        const size_t nl = sh.count(j->goff), nb = sh.items();
        std::vector<uint8_t> kd(nl), fr(frozen ? nl : 0);
        std::vector<double> in(2 * nl), out(3 * nl + HMC_SC_COUNT * nb), tr(nl * rows);
        std::vector<int32_t> inf(nb);
        sh.gather(j->goff, kind, kd.data());
        if (frozen) sh.gather(j->goff, frozen, fr.data());
        sh.gather(j->goff, z0, in.data());
        sh.gather(j->goff, mom, in.data() + nl);
        double *const lat = out.data(), *const sc = lat + 3 * nl;   // z1 | mom1 | theta1, then the scalars
        const ngp_status st = grad_leaf_hmc(
            sh.leaf, cfg, kd.data(), frozen ? fr.data() : nullptr, in.data(), in.data() + nl,
            HmcOut{lat, lat + nl, lat + 2 * nl, sc, sc + nb, sc + 2 * nb, sc + 3 * nb, sc + 4 * nb,
                   inf.data(), z_trace ? tr.data() : nullptr});
        if (st) return st;
        double *const lat_to[3] = {z1, mom1, theta1}, *const sc_to[HMC_SC_COUNT] = {U0, K0, U1, K1, logml1};
        for (int a = 0; a < 3; ++a) sh.scatter(j->goff, lat + (size_t)a * nl, lat_to[a]);
        for (size_t r = 0; r < rows; ++r) sh.scatter(j->goff, tr.data() + r * nl, z_trace + r * NL);
        for (int a = 0; a < HMC_SC_COUNT; ++a) sh.scatter_items(sc + (size_t)a * nb, sc_to[a]);
        sh.scatter_items(inf.data(), info1);
    }
    j->host_copy_follows(theta1, j->goff, nullptr);
    return NGP_OK;
}

extern "C" ngp_status ngp_grad_job_info(const ngp_grad_job *j, int32_t *out5) {
    if (!j || !out5) return NGP_ERR_ARG;
    out5[0] = j->gen ? j->gen->B : 0;
    out5[1] = j->gen ? j->gen->last_chunk : 0;
    out5[2] = j->toep ? j->toep->B : 0;
    out5[3] = j->toep ? j->toep->last_chunk : 0;
    out5[4] = j->side_by_side ? 1 : 0;
    return NGP_OK;
}

extern "C" void ngp_grad_job_destroy(ngp_grad_job *j) {
    if (!j) return;
    grad_leaf_destroy(j->gen);
    grad_leaf_destroy(j->toep);
    delete j;
}

// route: stage under this spec and these switches instead of the context's current ones
static ngp_status logml_grad_direct(ngp_ctx *c, int32_t B, const ngp_kernel *kernels, int32_t n,
                                    const double *t, const double *y, int64_t ldy,
                                    const double *const *yrows, double *logml, double *grad,
                                    int32_t *info, const GradRoute *route = nullptr) {
    if (!grad) return NGP_ERR_ARG;
    ngp_grad_job *j = nullptr;
    ngp_status st = grad_stage_impl(c, B, kernels, n, t, y, ldy, yrows, &j, false, route);
    if (st) return st;
    st = grad_job_run_resident(j, logml, grad, info);
    ngp_grad_job_destroy(j);
    return st;
}

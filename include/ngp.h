/*
 * ngp.h — C-ABI of the MI355X-native GP inference core ("libngp").
 *
 * This is the drop-in boundary for the ONE hot path NowcastAutoGP delegates to
 * AutoGP.jl: per-particle covariance assembly from a kernel tree -> Cholesky ->
 * log-marginal-likelihood -> posterior-predictive solves, batched over SMC
 * particles x nowcast scenarios.  Reference call sites (paths relative to the
 * reference checkout):
 *     src/make_and_fit_model.jl:84-91   GPModel(...), linear_schedule, fit_smc!
 *     src/forecasting.jl:46-47,65-67  predict_mvn + rand
 *     src/forecasting.jl:133-149          GPModel(dict), add_data!, maybe_resample!,
 *                                         mcmc_structure!, mcmc_parameters!
 * The reference has no FFI of its own (it is pure Julia on AutoGP.jl); the
 * entry points below are what a Julia `ccall` / Python `ctypes` shim binds in
 * place of AutoGP's internal covariance/Cholesky/logpdf arithmetic.  See
 * INTEGRATION.md for the binding stubs.
 *
 * Conventions
 *   - plain C, no exceptions cross the boundary; every function returns an
 *     ngp_status (0 = ok, <0 = bad argument, >0 = HIP runtime error code).
 *   - all pointers are caller-owned HOST memory, valid for the duration of the
 *     call (or, for staged jobs, until ngp_job_run returns for inputs and
 *     ngp_job_fetch returns for outputs); the library retains none of them.
 *   - Float64 everywhere (src/forecasting.jl:62); dense outputs are row-major
 *     and symmetric where that applies, so Julia's column-major view is the same
 *     matrix.
 *   - numerical failure is reported PER ITEM in info[] with LAPACK potrf
 *     semantics (k > 0: leading minor k is not positive definite), which the
 *     shim rethrows as PosDefException(k) (src/make_and_fit_model.jl:6-8).  Every output
 *     of an item with info > 0 that depends on the failed minor is non-finite (logml of the
 *     n + d points, mu, sigma; logml_base too unless k > n); other items are not affected.
 *   - re-entrant: may be entered concurrently from many host threads
 *     (Threads.@spawn per scenario, src/forecasting.jl:131-132); device work of one
 *     ctx is serialised by a blocking mutex, never a spin, and concurrent one-shot
 *     calls on the same dates are combined into one launch sequence ("concurrent
 *     callers" below).
 */
#ifndef NGP_H
#define NGP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- kernel grammar: opcode numbering follows AutoGP.GP.GPConfig ---------
 * (docs/src/vignettes/setting-priors.md:229-236 in the reference).            */
enum {
    NGP_OP_CONSTANT     = 1, /* params: value                                 */
    NGP_OP_LINEAR       = 2, /* params: intercept, bias, amplitude            */
    NGP_OP_SQEXP        = 3, /* params: lengthscale, amplitude                */
    NGP_OP_GAMMAEXP     = 4, /* params: lengthscale, gamma, amplitude         */
    NGP_OP_PERIODIC     = 5, /* params: lengthscale, period, amplitude        */
    NGP_OP_PLUS         = 6, /* binary, no params                             */
    NGP_OP_TIMES        = 7, /* binary, no params                             */
    NGP_OP_CHANGEPOINT  = 8  /* binary, params: location, scale               */
};

#define NGP_MAX_OPS    64  /* nodes per kernel tree                            */
#define NGP_MAX_PARAMS 96  /* continuous parameters per kernel tree            */
#define NGP_MAX_STACK  16  /* RPN evaluation stack depth                       */
#define NGP_MAX_AUX    192 /* appended + forecast rows per item (d_tail+d+m+1) */
/* Size limits beyond these (NGP_ERR_TOO_LARGE): a series of more than 16,256 points (11,520 for
 * ngp_logml_grad_batch) — an item's factor storage is addressed with 32-bit byte offsets; a
 * resident factor of more than 65,535 particles.  Batches of any size are cut into chunks that
 * fit the device memory; series longer than 8,319 points run NGP_PREC_MIXED jobs in fp64.        */

/* Formula variants.  AutoGP.jl's source is not available in the build
 * container, so the per-node formulas are restated from memory (SURVEY.md
 * Appendix B); each doubtful choice is a data-driven flag so that correcting
 * it is a one-line spec change + fixture regeneration, not a kernel rewrite. */
typedef struct ngp_spec {
    int32_t se_form;       /* 0: a*exp(-0.5*d^2/l^2)       1: a*exp(-0.5*d^2/l)        */
    int32_t periodic_form; /* 0: a*exp(-(2/l^2)*sin^2(pi*d/p))  1: a*exp(-(2/l)*sin^2(pi*d/p)) */
    int32_t cp_form;       /* 0: sigma(x)=.5*(1+tanh((loc-x)/scale))  1: tanh((x-loc)/scale) */
    int32_t precision;     /* NGP_PREC_F64 (default) or NGP_PREC_MIXED, see below          */
    double  jitter;        /* added to the diagonal next to the noise variance */
    /* ---- NGP_PREC_MIXED only (BASELINE config C5: long histories) ---------------------
     * The trailing updates of the blocked Cholesky run on the fp32 matrix cores wherever
     * that is provably harmless and in fp64 elsewhere: a workgroup multiplies two tiles of
     * the column pair (A) with two row tiles (B), 64x64 tiles of L each, and a k-tile of
     * those four products goes through v_mfma_f32_32x32x2_f32 (operands rounded to fp32) iff
     *     64 * 2^-24 * max|A tiles| * max|B tiles|  <=  mixed_tau * (noise + jitter),
     * the maxima taken over BOTH tiles of each pair (stricter than a rule per single
     * product), i.e. iff the rounding error of each is below mixed_tau of the smallest
     * pivot the matrix can have; everything else (the diagonal blocks, the panel solves,
     * the accumulators and the stored factor) stays fp64.  The Gram matrix X K^-1 X' of the appended / forecast
     * / data rows is then refined against the fp64 covariance (G <- A X' + (X - A K) A',
     * A += (X - A K) (L L')^-1) until the predicted remaining relative error is below
     * refine_tol or refine_max steps were taken; an item that does not get there is
     * reported with info = NGP_INFO_NOT_REFINED.  log det comes from the factor itself.
     * Series of fewer than 128 or more than 8,319 points, gradient jobs and resident
     * factors run in fp64 whatever this field says (ngp_job_mixed_stats: frac_f32 = 0).  */
    double  mixed_tau;     /* default 1e-6                                              */
    double  refine_tol;    /* default 1e-9                                              */
    int32_t refine_max;    /* default 3 (0: no refinement)                              */
    int32_t reserved;
} ngp_spec;
enum { NGP_PREC_F64 = 0, NGP_PREC_MIXED = 1 };
/* info[] < 0: not a pivot index */
#define NGP_INFO_NOT_REFINED (-2)
#define NGP_INFO_NOT_FINITE (-3)      /* ngp_mixture_crps_mapped: the score is infinite / undefined */
#define NGP_INFO_NOT_CONVERGED (-4)   /* ngp_mixture_crps_mapped: panel cap reached, values returned */

/* One particle's covariance kernel: the tree in postfix (RPN) order
 * (left subtree, right subtree, operator); params are consumed in RPN order. */
typedef struct ngp_kernel {
    int32_t        n_ops;
    int32_t        n_params;
    const int32_t *ops;     /* [n_ops] opcodes 1..8                            */
    const double  *params;  /* [n_params]                                      */
    double         noise;   /* observation-noise variance on the diagonal      */
} ngp_kernel;

typedef int32_t ngp_status;
enum {
    NGP_OK               =  0,
    NGP_ERR_ARG          = -1, /* null pointer / negative size                 */
    NGP_ERR_PROGRAM      = -2, /* malformed kernel program                     */
    NGP_ERR_TOO_LARGE    = -3, /* exceeds NGP_MAX_* or device memory           */
    NGP_ERR_NO_DEVICE    = -4, /* no HIP device / extension not usable         */
    NGP_ERR_STATE        = -5, /* job used out of order                        */
    NGP_ERR_UNAVAILABLE  = -6  /* optional component missing (librccl.so)      */
};

typedef struct ngp_ctx ngp_ctx;
typedef struct ngp_job ngp_job;

/* ---- context ------------------------------------------------------------- */
ngp_status  ngp_ctx_create(int32_t device, ngp_ctx **out);
void        ngp_ctx_destroy(ngp_ctx *ctx);
ngp_status  ngp_set_spec(ngp_ctx *ctx, const ngp_spec *spec);
ngp_status  ngp_get_spec(const ngp_ctx *ctx, ngp_spec *spec);
void        ngp_default_spec(ngp_spec *spec);
const char *ngp_strerror(ngp_status st);
const char *ngp_version(void);
/* validates a kernel program (arity, stack depth, parameter count) */
ngp_status  ngp_kernel_check(const ngp_kernel *k);

/* ---- concurrent callers ----------------------------------------------------
 * The reference enters this boundary from one task per nowcast scenario
 * (Threads.@spawn, src/forecasting.jl:131-159): D tasks with the P particles of their own clone
 * each, all on the same dates.  One-shot calls that arrive while the device is busy —
 * ngp_logml_batch, ngp_predict_batch, ngp_logml_grad_batch, ngp_mixture_sample (S = 1) — are
 * therefore COMBINED: the calling thread that finds nobody serving takes every pending request,
 * and requests of the same entry point on bytewise identical dates (same n, same forecast dates
 * and flags) run as ONE launch sequence of sum(B) items with per-item observation rows; every
 * caller gets its own results and status.  Gradient requests combine only with requests of the
 * same spec and switches (ngp_set_spec, ngp_set_structured_storage, ngp_set_batch_invariant,
 * ngp_set_short_series_path), and the group runs under them: a ngp_grad_job_run brings the ones
 * its job was staged under, a ngp_logml_grad_batch the context's current ones.  A call that arrives alone runs exactly as before;
 * only a caller whose predecessors came in company gives that company at most 200 microseconds to
 * arrive before it serves (tasks woken together by one sequence come back within microseconds of
 * each other), and a wait that was in vain is not repeated.  src/forecasting.jl needs no edit to
 * reach batches of P x (concurrent tasks) items.  A result is the one a single call over the combined
 * items would give: equal to the caller's own call up to the last bits (batch size decides
 * launch shapes and therefore summation order, as it always did — see DESIGN.md section 4.14).
 * ngp_grad_job_hmc (a whole trajectory on one job) takes the context's lock from its first launch
 * to its results and is never combined: callers that arrive meanwhile wait as for any other call.
 * ngp_set_combining(ctx, 0) switches it off (every call then waits for ctx's lock and runs alone);
 * 1 (default) is as described; 2 combines what is pending but never waits for company (without the
 * wait a convoy of T tasks alternates between groups of 1 and T - 1: measured 1.45 x slower at
 * 8 x 24 items, n = 208 (380 launch sequences instead of 200), 1.08 x at 16 x 64 items, n = 2048 —
 * profiles/r04/combine_linger_ab.txt).
 * A group of logml or predictive requests that carry THE SAME kernels (byte for byte) and whose
 * observations differ only in their last few points — the scenario tasks of the reference's default
 * mode, n_mcmc = n_hmc = 0 (src/forecasting.jl:120, 133-155): clones of one model, each with its own
 * nowcast values on shared dates (src/create_nowcast_data.jl:36-37) — is served by ONE factorisation
 * per particle with the tasks' last points as scenarios (the arithmetic of ngp_nowcast_batch), not by
 * one factorisation per (particle, task): K does not depend on y.  Results equal the caller's own
 * call to rounding (1e-8 on predictive moments in the tests, condition-aware).
 * ngp_combine_stats: out6 = { requests seen, launch sequences run for them, largest group,
 * requests that shared a sequence with at least one other, requests served from one shared
 * factorisation per particle, reserved }; reset != 0 clears the counters.                      */
ngp_status ngp_set_combining(ngp_ctx *ctx, int32_t on);
/* Batch-invariant arithmetic (off by default; applies to jobs staged after the call).  By default
 * a few decisions follow the size of the batch an item travels in, for speed: late block columns of
 * a small chunk are split along k, a small mixed gradient batch runs all its items on the general
 * leaf while a large one gives its stationary trees to the Toeplitz leaf, the contraction of a small
 * batch cuts its tiles finer and picks one kernel shape for all its trees, a single-chunk job's
 * epilogue reads resident tables.  Each of these changes a summation order or an arithmetic path:
 * results agree to rounding (1e-13 on logml, 1e-11 on gradients in the tests) but not bit for bit, so
 * what a caller gets depends on who shared its launch sequence — with combining, on thread timing.
 * With this option on, every such decision is taken from the item and the series alone: an item's
 * outputs are the same bits whether it is evaluated alone, in a lockstep P x D call or in a
 * combined group (tests/test_combine_gpu.py, tests/test_lockstep_gpu.py), at the price of the
 * small-batch shortcuts (64 items at n = 2048: see DESIGN.md section 4.14).                    */
ngp_status ngp_set_batch_invariant(ngp_ctx *ctx, int32_t on);
ngp_status ngp_combine_stats(ngp_ctx *ctx, int64_t *out6, int32_t reset);

/* ---- covariance assembly (diagnostic / small blocks) ---------------------
 * out[b] (n1 x n2, row-major) = k_b(t1_i, t2_j) (+ (noise_b + jitter) on the
 * diagonal i==j when add_diag != 0).  Replaces AutoGP's covariance-matrix
 * builder used under fit_smc!/predict_mvn (src/make_and_fit_model.jl:91,
 * src/forecasting.jl:46).                                                   */
ngp_status ngp_cov_batch(ngp_ctx *ctx, int32_t B, const ngp_kernel *kernels,
                         int32_t n1, const double *t1, int32_t n2, const double *t2,
                         int32_t add_diag, double *out);

/* ---- log marginal likelihood --------------------------------------------
 * logml[b] = log N(y_b | 0, K_b(t,t) + (noise_b + jitter) I), b = 0..B-1.
 * y is [B x n] with row stride ldy (ldy == 0: one y shared by all items).
 * This is the per-particle evaluation inside fit_smc! / add_data! /
 * mcmc_structure! (src/make_and_fit_model.jl:91, src/forecasting.jl:135,146). */
ngp_status ngp_logml_batch(ngp_ctx *ctx, int32_t B, const ngp_kernel *kernels,
                           int32_t n, const double *t, const double *y, int64_t ldy,
                           double *logml, int32_t *info);

/* ---- posterior predictive ------------------------------------------------
 * Per item: mu[b] (m), sigma[b] (m x m) of  f(t_new) | y_b  (+ observation
 * noise on the new points when noise_on_new != 0), and logml[b] (may be NULL).
 * Replaces the per-particle conditional MVN inside AutoGP.predict_mvn
 * (src/forecasting.jl:46,66).                                              */
ngp_status ngp_predict_batch(ngp_ctx *ctx, int32_t B, const ngp_kernel *kernels,
                             int32_t n, const double *t, const double *y, int64_t ldy,
                             int32_t m, const double *t_new, int32_t noise_on_new,
                             double *mu, double *sigma, double *logml, int32_t *info);

/* ---- nowcast fan-out ------------------------------------------------------
 * The whole body of forecast_with_nowcasts' per-scenario task for the default
 * n_mcmc = n_hmc = 0 path (src/forecasting.jl:133-155), for P particles and D
 * scenarios at once.  All scenarios share the appended dates
 * (src/create_nowcast_data.jl:36-37), and K does not depend on y, so each
 * particle is factorised ONCE; per scenario only the d appended observations
 * differ.
 *   in : P kernels; base data (t[n], y[n]); appended times t_add[d];
 *        y_add [D x d] row-major; forecast times t_new[m].
 *   out: logml_base[P]      log p(y | particle)                 (n points)
 *        logml_full[P x D]  log p(y, y_add_s | particle)        (n+d points)
 *                           -> add_data! incremental weight = full - base
 *        mu   [P x D x m]   predictive mean given (y, y_add_s)
 *        sigma[P x m x m]   predictive covariance (scenario-independent)
 *        info [P]
 * Any output pointer may be NULL.                                            */
ngp_status ngp_nowcast_batch(ngp_ctx *ctx, int32_t P, const ngp_kernel *kernels,
                             int32_t n, const double *t, const double *y,
                             int32_t d, const double *t_add,
                             int32_t D, const double *y_add,
                             int32_t m, const double *t_new, int32_t noise_on_new,
                             double *logml_base, double *logml_full,
                             double *mu, double *sigma, int32_t *info);

/* ---- gradient of the log marginal likelihood ------------------------------
 * grad[b] has n_params_b + 1 entries: d logml / d params (RPN order) followed
 * by d logml / d noise; items are packed back to back (offsets = running sum of
 * n_params_b + 1).  Needed by the HMC moves of mcmc_parameters! / fit_smc!
 * (src/forecasting.jl:65,148; src/make_and_fit_model.jl:91).               */
ngp_status ngp_logml_grad_batch(ngp_ctx *ctx, int32_t B, const ngp_kernel *kernels,
                                int32_t n, const double *t, const double *y, int64_t ldy,
                                double *logml, double *grad, int32_t *info);

/* The same evaluation with its inputs resident on the device: trees, dates and observations are
 * staged once (ngp_grad_stage: exactly ngp_logml_grad_batch's arguments), every
 * ngp_grad_job_run evaluates logml and gradient for the parameters the job currently holds, and
 * ngp_grad_job_set_params replaces them between runs — `params`: the items' parameter vectors
 * back to back in the caller's (RPN) order, n_params_b each; noise[B].  The leapfrog steps of
 * one HMC move (src/forecasting.jl:65,148; src/make_and_fit_model.jl:91) change nothing but the
 * parameters: per step only they cross the bus (1 KiB per item instead of the observations and
 * the compiled trees).  ngp_logml_grad_batch = stage + run + destroy; a run's outputs are those
 * of the one-shot call, bit for bit.  The job keeps the spec it was staged under; it holds only
 * its inputs and results between runs (the factor storage is taken per run).                  */
typedef struct ngp_grad_job ngp_grad_job;
ngp_status ngp_grad_stage(ngp_ctx *ctx, int32_t B, const ngp_kernel *kernels, int32_t n,
                          const double *t, const double *y, int64_t ldy, ngp_grad_job **out);
ngp_status ngp_grad_job_set_params(ngp_grad_job *job, const double *params, const double *noise);
ngp_status ngp_grad_job_run(ngp_grad_job *job, double *logml, double *grad, int32_t *info);
/* How the job is carried (diagnostic; tests use it to pick the first and last item of every chunk):
 * out5 = { items of the general leaf, items per memory-driven chunk of its last run (0 before the
 * first), items of the Toeplitz leaf (stationary trees on a regular series, ngp_set_structured_storage),
 * items per chunk of its last run, 1 if the two leaves run side by side }.  Leaf items keep the
 * caller's order.                                                                                */
ngp_status ngp_grad_job_info(const ngp_grad_job *job, int32_t *out5);
/* One whole HMC leapfrog trajectory of every item of a staged job in one call: n_leapfrog + 1
 * gradient evaluations with the leapfrog update between them on the device, one synchronisation,
 * one copy back (mcmc_parameters!, src/forecasting.jl:65,148: one call per move instead of one per
 * leapfrog).  Latents are laid out as the gradient is: per item n_params_b entries in the caller's
 * (RPN) order followed by the noise latent, items back to back.  The arithmetic is that of the
 * Python mirror's autogp._hmc_move / potential, operation for operation:
 *   evaluation at z: a non-finite z is replaced for the evaluation (NaN -> 0, +-inf -> +-50);
 *     theta(z) by kind — real: z; unit: sigmoid(z); gamma: 2 sigmoid(mu + sigma z); period,
 *     wildcard: exp(mu + sigma z) — with the argument clamped to +-700 (sigmoid) / +-300 (exp);
 *     theta clipped to +-1e6, positive kinds >= 1e-12, gamma to [1e-9, 2 - 1e-9], unit to
 *     [1e-9, 1 - 1e-9]; ok = info == 0, logml finite, every gradient entry finite;
 *     U = ok ? -logml + z'z / 2 : +inf;  dU = ok ? -grad * dtheta/dz + z : 0, and 0 where frozen.
 *   pm = mom - eps/2 dU(z0); n_leapfrog times: z += eps pm, evaluate, pm -= eps dU (the last: eps/2).
 *   K0 = mom'mom / 2, K1 = pm'pm / 2; U0 / U1, logml1, info1: first / last evaluation; theta1: the
 *   parameters of the last evaluation; z1 = z, mom1 = pm; z_trace row s: the z of evaluation s.
 * An item that fails at an intermediate evaluation keeps moving (dU = 0 there).  The library draws
 * nothing: momenta and the accept decision stay with the caller.  A job carried by two leaves runs
 * the trajectory of the general leaf, then that of the Toeplitz leaf (items are independent).
 * Every evaluation is the launch sequence of ngp_grad_job_run: its logml / gradient are the bits a
 * run gives for the same parameters.  After the call the job holds the parameters of the last
 * evaluation (theta1): a following ngp_grad_job_run evaluates exactly those.  The call holds the
 * context's lock for the whole trajectory of a leaf and is not combined with concurrent callers; a
 * job on two leaves takes the lock once per leaf, so another caller's work may run between the two
 * trajectories (never inside one).  If the second leaf fails after the first succeeded, the call
 * returns the error, the outputs are not valid, and the items of the first leaf already hold their
 * last parameters on the device while the job's one-shot form still holds the old ones: send
 * parameters again (ngp_grad_job_set_params) before the job is run.
 * NGP_ERR_ARG: a null pointer, n_leapfrog < 1, a non-finite eps, a kind above 4, prior_sigma <= 0
 * (or a non-finite prior entry) for a kind in use.  NGP_ERR_TOO_LARGE: n_leapfrog above 65,536
 * (the library's limit on one call; the trace alone would be 65,537 rows), or no room for the
 * working storage or the arena.  The step kernel is booked under profile class 4 together with
 * the fills and the tables kernel of the evaluations: n_leapfrog + 2 more launch records there. */
typedef struct {
    int32_t n_leapfrog;            /* >= 1 */
    double  eps;
    double  prior_mu[5], prior_sigma[5];   /* indexed by latent kind; kinds 0 and 1 ignore them */
} ngp_hmc_config;
/* cfg: const void * to ONE ngp_hmc_config; kind / frozen: const void * to one byte (uint8_t) per
 * latent — declared so for the reason given at ngp_mixture_path_targets (the header's parameter
 * types stay scalars, arrays of scalars, handles and the three mirrored structs).               */
ngp_status ngp_grad_job_hmc(ngp_grad_job *job, const void *cfg,
                            const void *kind,    /* per latent: 0 real, 1 unit, 2 gamma, 3 period, 4 wildcard */
                            const void *frozen,  /* per latent, may be NULL: dU forced to 0 (fixed noise) */
                            const double *z0, const double *mom,   /* per latent */
                            double *z1, double *mom1, double *theta1,  /* per latent, out */
                            double *U0, double *K0, double *U1, double *K1, double *logml1, /* [B] */
                            int32_t *info1,          /* [B] info of the LAST evaluation */
                            double *z_trace);        /* may be NULL: [n_leapfrog + 1][latents] */
void       ngp_grad_job_destroy(ngp_grad_job *job);

/* ---- particle weights -----------------------------------------------------
 * maybe_resample! arithmetic (src/forecasting.jl:138-141): normalise P
 * log-weights (logsumexp), effective sample size 1 / sum w^2.  In a multi-GPU
 * run the caller all-gathers the per-rank log-weights first (the only
 * collective on the path) and passes the gathered vector.
 * w_norm (P, may be NULL), ess, log_norm (log sum exp logw) out.              */
ngp_status ngp_weights_normalize(int32_t P, const double *logw,
                                 double *w_norm, double *ess, double *log_norm);
/* The same for D weight vectors at once — the D scenario clones forecast_with_nowcasts
 * advances together (src/forecasting.jl:131-141): logw and w_norm are [P x D] row-major (one
 * COLUMN per scenario, the layout of the all-gathered [P_local, D] shards), ess and log_norm
 * are [D].  Column s equals ngp_weights_normalize on that column.                          */
ngp_status ngp_weights_normalize_cols(int32_t P, int32_t D, const double *logw,
                                      double *w_norm, double *ess, double *log_norm);

/* ---- the collective of the path, for hosts without a collective library --------------
 * maybe_resample! is the only step of the hot path that needs every rank's particles
 * (src/forecasting.jl:138-141): the P_total log-weights of every scenario.  A Julia host that
 * runs one process per GPU has no torch.distributed; these entry points give it that one exchange
 * over RCCL (xGMI inside a node).  librccl.so is opened at run time (no link-time dependency);
 * without it every call returns NGP_ERR_UNAVAILABLE and the host must gather the weights itself
 * and call ngp_weights_normalize_cols.
 *   ngp_comm_unique_id   rank 0 makes the 128-byte id (ncclGetUniqueId) and hands it to the other
 *                        ranks by the host's own means (a file, a socket, MPI, Julia Distributed)
 *   ngp_comm_create      collective over all ranks (ncclCommInitRank) on the context's device
 *   ngp_weights_allgather_normalize
 *        particles are block-partitioned over the ranks, remainder to the low ranks; this rank
 *        passes its rows logw_local [P_local x D] (D scenario columns, row-major); ONE all-gather
 *        of padded shards, then the normalisation of ngp_weights_normalize_cols on every rank:
 *        w_local [P_local x D] (may be NULL), w_all [P_total x D] (may be NULL: what resampling
 *        needs), ess [D], log_norm [D] (may be NULL).  Identical on every rank.
 *        Every rank must own at least one particle: P_total >= world (NGP_ERR_ARG otherwise).
 *        A non-zero return on ANY rank is fatal for the communicator — the others may be inside
 *        the all-gather: destroy it and make a new one.  ngp_comm_create gives this process's
 *        cached device blocks back before its ONE ncclCommInitRank (a collective: never retried
 *        by one rank alone).
 *   ngp_weights_unpad_normalize
 *        the host half of that exchange, for a host that brings its own all-gather: `padded` is
 *        what gathering equally sized zero-padded shards delivers — world blocks of pmax x D doubles,
 *        pmax = rows of rank 0 (ngp_shard), block r = rank r's rows, then padding — and comes out
 *        as w_all [P_total x D] (may be NULL), ess [D] (may be NULL), log_norm [D] (may be NULL).  */
typedef struct ngp_comm ngp_comm;
/* the block partition itself (host-only arithmetic): rank's first global particle and its count */
ngp_status ngp_shard(int32_t P_total, int32_t world, int32_t rank, int32_t *first, int32_t *rows);
ngp_status ngp_comm_unique_id(void *id128);
ngp_status ngp_comm_create(ngp_ctx *ctx, const void *id128, int32_t rank, int32_t world,
                           ngp_comm **out);
void       ngp_comm_destroy(ngp_comm *comm);
ngp_status ngp_weights_allgather_normalize(ngp_comm *comm, int32_t P_total, int32_t D,
                                           const double *logw_local, double *w_local,
                                           double *w_all, double *ess, double *log_norm);
ngp_status ngp_weights_unpad_normalize(int32_t P_total, int32_t world, int32_t D,
                                       const double *padded, double *w_all, double *ess,
                                       double *log_norm);

/* ---- staged execution (inputs resident in HBM before the timed region) ----
 * stage  : validate, allocate device buffers, copy inputs host -> device
 * run    : enqueue every kernel of the job and wait for completion
 * fetch  : copy outputs device -> host (same output arguments as the one-shot
 *          entry point that created the job; NULL pointers are skipped)
 * The one-shot entry points above are stage + run + fetch + destroy.          */
ngp_status ngp_logml_stage(ngp_ctx *ctx, int32_t B, const ngp_kernel *kernels,
                           int32_t n, const double *t, const double *y, int64_t ldy,
                           ngp_job **job);
ngp_status ngp_predict_stage(ngp_ctx *ctx, int32_t B, const ngp_kernel *kernels,
                             int32_t n, const double *t, const double *y, int64_t ldy,
                             int32_t m, const double *t_new, int32_t noise_on_new,
                             ngp_job **job);
ngp_status ngp_nowcast_stage(ngp_ctx *ctx, int32_t P, const ngp_kernel *kernels,
                             int32_t n, const double *t, const double *y,
                             int32_t d, const double *t_add,
                             int32_t D, const double *y_add,
                             int32_t m, const double *t_new, int32_t noise_on_new,
                             ngp_job **job);
ngp_status ngp_job_run(ngp_job *job);
ngp_status ngp_job_fetch(ngp_job *job, double *logml_base, double *logml_full,
                         double *mu, double *sigma, int32_t *info);
/* NGP_PREC_MIXED jobs, after ngp_job_run (any pointer may be NULL; all [B]):
 *   refine_steps  refinement steps taken for the item (0 for an fp64 job)
 *   refine_delta  relative size of the last correction applied to its Gram matrix
 *   frac_f32      share of its tile products that ran on the fp32 matrix cores         */
ngp_status ngp_job_mixed_stats(ngp_job *job, int32_t *refine_steps, double *refine_delta,
                               double *frac_f32);
void       ngp_job_destroy(ngp_job *job);

/* ---- mixture sampling on the device -------------
 * predict_mvn(...) |> rand of the reference (src/forecasting.jl:47, 67) for S
 * mixtures over the same P components at once (S = nowcast scenarios): component
 * k ~ Categorical(w[s][.]), then  mu[k][s][.] + chol(sigma[k]) z,  z ~ N(0, I).
 *   w     [S x P]      mixture weights, each row sums to 1 (ngp_weights_normalize)
 *   mu    [P x S x m]  component means   (layout of ngp_nowcast_batch's mu)
 *   sigma [P x m x m]  component covariances, shared by the S mixtures
 *   out   [S x draws x m]; comp [S x draws] (may be NULL) the component drawn;
 *   info  [P] (may be NULL): 0, or the first non-positive pivot of chol(sigma[k])
 * Randomness: Philox4x32-10 (counter = (draw, scenario, block, 0), key = seed):
 * reproducible for a given seed on any device and by the numpy restatement in
 * oracle/, NOT against Julia's Xoshiro stream — the reference's own tests only
 * check shapes and ranges of draws.  m <= NGP_MAX_AUX.     */
ngp_status ngp_mixture_sample(ngp_ctx *ctx, int32_t P, int32_t S, int32_t m,
                              const double *w, const double *mu, const double *sigma,
                              int32_t draws, uint64_t seed,
                              double *out, int32_t *comp, int32_t *info);
/* S INDEPENDENT mixtures of P components each — the scenario clones after a refinement
 * (mcmc_structure! / mcmc_parameters!, src/forecasting.jl:145-148) no longer share their
 * particles:
 *   w [S x P], mu [S x P x m], sigma [S x P x m x m], seeds [S],
 *   out [S x draws x m], comp [S x draws] (may be NULL), info [S x P] (may be NULL).
 * Mixture s is keyed by seeds[s] with scenario counter 0: it draws exactly what
 * ngp_mixture_sample(P, S = 1, ..., seed = seeds[s]) draws, so one call replaces S calls.   */
ngp_status ngp_mixture_sample_indep(ngp_ctx *ctx, int32_t P, int32_t S, int32_t m,
                                    const double *w, const double *mu, const double *sigma,
                                    int32_t draws, const uint64_t *seeds,
                                    double *out, int32_t *comp, int32_t *info);

/* ---- exact summaries of the forecast mixture (per-date marginals) ------------------
 * What the users of the reference compute from the draws — quantile(fc, probs) per forecast date
 * and the CRPS against what was later observed (docs/vignettes/getting-started.jl:433-746) — in
 * closed form from the mixture itself, without draws and without the m x m factor of any
 * covariance.  A mixture is a flat list of C components over m dates; the caller pools scenarios
 * (component (s, k) of S scenarios gets weight w[s][k] / S):
 *   w   [C]      weights, >= 0, finite, summing to 1 (as for ngp_mixture_sample; not renormalised)
 *   mu  [C x m]  marginal means, component-major
 *   var [C x m]  marginal variances (the diagonal of each component's covariance)
 * Per date j, with sd^2 = var:
 *   F_j(x)    = sum_c w_c Phi((x - mu_cj) / sd_cj)
 *   q_j(p)    : F_j(q) = p                                        (0 < p < 1)
 *   A(d, v)   = d erf(d / sqrt(2 v)) + sqrt(2 v / pi) exp(-d^2 / (2 v))         ( = E|N(d, v)| )
 *   CRPS_j(y) = sum_c w_c A(y - mu_cj, var_cj)
 *               - 1/2 sum_c sum_c' w_c w_c' A(mu_cj - mu_c'j, var_cj + var_c'j)
 * (E|X - y| - 1/2 E|X - X'| in closed form; Grimit et al. 2006).  ngp_mixture_cdf with x = y is
 * the PIT value.
 *   ngp_mixture_cdf       x [m x K] (K points per date)  -> cdf  [m x K]
 *   ngp_mixture_quantiles probs [Q], each in (0, 1)      -> q    [m x Q]
 *   ngp_mixture_crps      y [m]                          -> crps [m]
 * "Exact" means: no sampling error — the result is the formula evaluated in fp64 (CDF to 1e-13
 * absolute; a quantile q satisfies |F(q) - p| <= 1e-13 + a few ulp of q times the density; CRPS to
 * 1e-12 of the size of the two sums it is the difference of), judged against a long double
 * evaluation in tests/.  Quantiles are non-decreasing in p and a level's result does not depend on
 * Q or on its position in probs.
 * Malformed calls are NGP_ERR_ARG before anything touches a device: null context or arrays; C, m,
 * K or Q < 1; a probs entry outside (0, 1); a negative or non-finite weight; weights all zero.
 * Numerical trouble is per date: info[j] = c + 1 for the first component c with w_c > 0 whose mean
 * is not finite or whose variance is not finite and positive at date j — that date's outputs are
 * NaN, other dates are not affected (0: fine).  Components with w_c = 0 are ignored, bad values
 * included.
 * Limits (NGP_ERR_TOO_LARGE): C <= 65,536 components, K and Q <= 4,096, m <= 65,535 dates and what
 * the device memory holds (24 C m bytes and, for the CRPS, 4 m (C / 256)^2) — NOT NGP_MAX_AUX: no
 * m x m object exists here.
 * Bitwise reproducible: the same inputs give the same bits on every call, a date's bits do not
 * depend on the other dates of the call (every sum runs in a fixed order; no floating-point
 * atomics).  Thread-safe like the other one-shot calls (the context's lock); these calls are not
 * combined with concurrent callers.                                                            */
ngp_status ngp_mixture_cdf(ngp_ctx *ctx, int32_t C, int32_t m, const double *w, const double *mu,
                           const double *var, int32_t K, const double *x, double *cdf,
                           int32_t *info);
ngp_status ngp_mixture_quantiles(ngp_ctx *ctx, int32_t C, int32_t m, const double *w,
                                 const double *mu, const double *var, int32_t Q,
                                 const double *probs, double *q, int32_t *info);
ngp_status ngp_mixture_crps(ngp_ctx *ctx, int32_t C, int32_t m, const double *w, const double *mu,
                            const double *var, const double *y, double *crps, int32_t *info);

/* ---- trajectory targets: functionals of whole sample paths on the original scale -------------
 * What the per-date summaries above cannot give — the total over the next k dates, the peak value,
 * the peak date, the probability that any date exceeds a threshold, the probability that date j1 is
 * above date j0 — has no closed form under a mixture of Gaussians followed by a Box-Cox, log or
 * logit inverse (reference src/transformations.jl:139-174): it needs paths.  These calls draw the
 * paths, transform them, reduce them and rank them on the device; only the summaries come back.
 *
 * Paths.  w, mu, sigma, draws, seed / seeds and their layouts are those of ngp_mixture_sample /
 * ngp_mixture_sample_indep; path (s, d) is the path that call draws for the same arguments (same
 * Philox counters, component pick and Box-Muller pairing), equal to it to rounding — bit equality
 * is not promised.  The N = S draws paths are pooled, as the reference's hcat pools them.
 * Inverse transformation.  Every path value is v = g(x), g as nowcast.get_transformations builds
 * its inverses, edge rules included:
 *   NGP_INV_IDENTITY     x
 *   NGP_INV_EXP          max(exp(x) - offset, 0)
 *   NGP_INV_LOGISTIC100  max(100 / (1 + exp(-x)) - offset, 0)
 *   NGP_INV_BOXCOX       with base = lam x + 1:
 *                          lam > 0:  max(base, 1e-10)^(1 / lam) - offset
 *                          lam < 0:  base^(1 / lam) - offset            where base > 1e-10,
 *                                    0                                  where base <= 0 (the pole),
 *                                    min(base^(1 / lam), cap) - offset  in between
 *                          lam = 0:  exp(x) - offset
 *                        then max(., 0), and a non-finite result becomes the largest finite double
 * -0.0 is stored as +0.0.
 * Targets, per path, over the inclusive window j0 .. j1 (0 <= j0 <= j1 < m):
 *   NGP_TARGET_SUM     sum of v_j, j ascending        NGP_TARGET_MAX     the window's maximum
 *   NGP_TARGET_DIFF    v[j1] - v[j0]                  NGP_TARGET_ARGMAX  first date j of the maximum
 *   NGP_TARGET_EXCEED  1 if any v_j > thr, else 0
 * Summaries over the N paths of target t:
 *   q [T x Q]     real-valued kinds (SUM, MAX, DIFF): the order statistic x_(k), k =
 *                 clamp((int64) ceil(probs[i] N), 1, N) — an exact selection, nothing interpolated
 *                 or approximated; a level's result does not depend on Q or on its position in
 *                 probs.  NaN for ARGMAX and EXCEED.
 *   mean [T]      the sum over the paths in a fixed order, over N (EXCEED: the probability; ARGMAX:
 *                 the mean date index)
 *   count [T]     paths with value > thr (DIFF with thr = 0: N P(increase)); EXCEED: the exceeding
 *                 paths; ARGMAX: 0
 *   hist [T x m]  ARGMAX: paths whose peak is at date j; zero outside the window and for other kinds
 *   values [T x N] (may be NULL) every path's target value, path (s, d) at s draws + d
 *   info          as ngp_mixture_sample: [P] ([S x P] for _indep), may be NULL; 0 or the first
 *                 non-positive pivot of chol(sigma[k]).  A failed component of positive weight makes
 *                 EVERY output of the call NaN (count and hist: 0) — its paths are pooled with the
 *                 others, so no summary is left that it has not touched.
 * Bitwise reproducible: the same inputs give the same bits on every call (fixed-order sums, no
 * floating-point atomics; integer atomics only where the order cannot matter).
 * NGP_ERR_ARG, before anything touches a device: null context or arrays (values and info may be
 * NULL; seeds may not); P, S, m, draws, T or Q < 1; a window outside [0, m) or with j0 > j1; an
 * unknown kind; a probs entry outside (0, 1); a non-finite thr, lam, offset or cap; NGP_INV_BOXCOX
 * with cap <= 0.  Limits (NGP_ERR_TOO_LARGE): m <= NGP_MAX_AUX, T <= 64, Q <= 64, N <= 2^31 - 1,
 * S P <= 2^31 - 1, and the 8 T N bytes of target values (kept on the device whether or not values
 * is asked for) must fit in device memory.
 * Thread-safe like the other one-shot calls (the context's lock); not combined with concurrent
 * callers; not counted in ngp_profile.
 * inv points to ONE ngp_inv_transform and targets to T ngp_path_target; the two parameters are
 * declared const void * because every other parameter type of this header is a scalar, an array of
 * scalars or an opaque handle, and the bindings that are checked against it (julia/NGPAutoGP.jl)
 * know only those.                                                                              */
enum { NGP_INV_IDENTITY = 0, NGP_INV_EXP = 1, NGP_INV_LOGISTIC100 = 2, NGP_INV_BOXCOX = 3 };
typedef struct ngp_inv_transform { int32_t kind; double lam, offset, cap; } ngp_inv_transform;
enum { NGP_TARGET_SUM = 0, NGP_TARGET_MAX = 1, NGP_TARGET_DIFF = 2,   /* real-valued */
       NGP_TARGET_ARGMAX = 3, NGP_TARGET_EXCEED = 4 };
typedef struct ngp_path_target { int32_t kind, j0, j1; double thr; } ngp_path_target;
ngp_status ngp_mixture_path_targets(ngp_ctx *ctx, int32_t P, int32_t S, int32_t m,
                                    const double *w, const double *mu, const double *sigma,
                                    int32_t draws, uint64_t seed, const void *inv,
                                    int32_t T, const void *targets, int32_t Q,
                                    const double *probs, double *q, double *mean, int64_t *count,
                                    int64_t *hist, double *values, int32_t *info);
ngp_status ngp_mixture_path_targets_indep(ngp_ctx *ctx, int32_t P, int32_t S, int32_t m,
                                          const double *w, const double *mu, const double *sigma,
                                          int32_t draws, const uint64_t *seeds,
                                          const void *inv, int32_t T,
                                          const void *targets, int32_t Q,
                                          const double *probs, double *q, double *mean,
                                          int64_t *count, int64_t *hist, double *values,
                                          int32_t *info);

/* ---- scores of the paths themselves: energy score and sample CRPS ----------------------------
 * A forecast is a matrix of draws, dates x N paths, and the reference scores every approach from
 * those draws: per date mean |X - y| minus half the mean of |X_i - X_j| over the pairs i < j
 * (docs/vignettes/getting-started.jl:689-702, after data_transform = log, :746) — an O(N^2) loop.
 * Over a window of dates the same expression with the Euclidean norm is the energy score, the
 * multivariate CRPS (Gneiting & Raftery 2007), which also sees paths of the wrong shape.
 * Per window w = [j0, j1] (inclusive), with u_i = s(x_i[j0..j1]), v = s(y[j0..j1]) and s
 * NGP_SCORE_NATURAL or NGP_SCORE_LOG with shift, as in ngp_mixture_crps_mapped:
 *   term_obs  = (1 / N) sum_i |u_i - v|_2
 *   term_pair = (1 / D) sum_(i < k) |u_i - u_k|_2      fair = 1: D = N (N - 1) / 2 (the vignette's
 *               estimator); fair = 0: D = N^2 / 2 (the V-statistic, as scoringutils computes it)
 *   es        = term_obs - term_pair / 2
 * A window of one date gives the sample CRPS of that date.  Windows may overlap or repeat.
 *   x [N x m]       paths on the ORIGINAL scale, path-major (row i is path i)
 *   y [m]           observations on the original scale
 *   win [W x 2]     j0, j1 of every window
 *   es [W]; term_obs [W], term_pair [W], info [W] may be NULL
 *   info[w]         0, or NGP_INFO_NOT_FINITE (-3), the window's outputs NaN: a path value or s(.)
 *                   of one inside the window is not finite — with NGP_SCORE_LOG every x + shift <= 0,
 *                   e.g. a clamp at 0 with shift 0 — or the values are finite but so large (about
 *                   1e154 apart and beyond; the largest finite double NGP_INV_BOXCOX caps at) that a
 *                   squared difference overflows and a sum is not finite.  Other windows are not
 *                   affected.
 * ngp_mixture_path_scores draws the N = S draws paths on the device with the sampler (indep = 0:
 * the layouts of ngp_mixture_sample, keyed by seeds[0]; indep = 1: those of
 * ngp_mixture_sample_indep, seeds [S]), applies the ONE ngp_inv_transform inv with the edge rules of
 * the trajectory targets and scores them as above; the paths never leave the device.  They are the
 * sampler's paths to rounding; bit equality with them is not promised.  chol_info ([P], or [S x P]
 * with indep = 1; may be NULL) is the sampler's info; a failed component of positive weight makes
 * every output NaN (info[w] = NGP_INFO_NOT_FINITE for every window).
 * Accuracy: the squared distance of a pair is summed from the DIFFERENCES u_ij - u_kj date by date,
 * never from a Gram product, so near-identical paths (1e6 + 1e-3 z; a clamp at exactly 0) keep
 * their distance.  Every sum runs in a fixed order and no chain of additions is longer than 2,048
 * terms: each term is within (2,048 + m + 8) 2^-53 relative of a long double evaluation of the
 * same s(.) values (2.6e-13 for m <= 192), tested to 1e-12 per term and 1e-12 (term_obs +
 * term_pair / 2) for es, the floor ngp_mixture_crps is granted.
 * Bitwise reproducible from call to call; a window's bits do not depend on the other windows of
 * the call (no floating-point atomics).
 * NGP_ERR_ARG, before anything touches a device: null context or required array; N, m, W or draws
 * < 1; fair = 1 with N < 2; a window outside [0, m) or with j0 > j1; scale, fair or indep not one
 * of their values; shift non-finite or < 0; a non-finite y, or a y where s(y) is undefined; for the
 * mixture form also what ngp_mixture_path_targets refuses (null w, mu, sigma, seeds, inv; P or S
 * < 1; an unknown inv.kind; non-finite lam, offset, cap; NGP_INV_BOXCOX with cap <= 0).
 * Limits (NGP_ERR_TOO_LARGE): N <= 2^20, W <= 4,096, m <= 65,535 (ensemble form) or NGP_MAX_AUX
 * (mixture form), and the paths (twice 8 N m bytes) plus the partial sums (8 W per 128 x 128 tile
 * of the pairs' upper triangle) must fit in device memory.
 * Thread-safe through the context's lock; not combined with concurrent callers; not counted in
 * ngp_profile.  (NGP_SCORE_* are declared with ngp_mixture_crps_mapped below.)                    */
ngp_status ngp_ensemble_scores(ngp_ctx *ctx, int32_t N, int32_t m, const double *x,
                               const double *y, int32_t scale, double shift, int32_t fair,
                               int32_t W, const int32_t *win, double *es, double *term_obs,
                               double *term_pair, int32_t *info);
ngp_status ngp_mixture_path_scores(ngp_ctx *ctx, int32_t P, int32_t S, int32_t m, const double *w,
                                   const double *mu, const double *sigma, int32_t indep,
                                   int32_t draws, const uint64_t *seeds, const void *inv,
                                   const double *y, int32_t scale, double shift, int32_t fair,
                                   int32_t W, const int32_t *win, double *es, double *term_obs,
                                   double *term_pair, int32_t *info, int32_t *chol_info);

/* ---- exact CRPS and mean on the natural and log scales ----------------------------------------
 * ngp_mixture_crps scores on the scale the mixture is Gaussian on.  The reference's vignette fits
 * on a Box-Cox scale, maps the draws back and scores crps(log(y), log.(X))
 * (docs/vignettes/getting-started.jl:704-747); hubs score on the natural and on the log scale.
 * Quantiles carry over through a monotone map, the CRPS and the mean do not — but both are
 * integrals in the mixture's own CDF.  With g ONE ngp_inv_transform, edge rules as above, and s the
 * score scale
 *   NGP_SCORE_NATURAL  s(v) = v            NGP_SCORE_LOG  s(v) = log(v + shift)
 * psi = s o g non-decreasing, Y = psi(X), yt = s(y) and x0 where psi crosses yt:
 *   CRPS(Y, yt) = int (F_X(x) - 1{x >= x0})^2 dpsi(x)  +  |yt - psi(x0)|
 *   E[Y]        = psi(x0) + int_{x > x0} (1 - F_X) dpsi - int_{x < x0} F_X dpsi
 * (the second term of the CRPS is nonzero only for a y the forecast cannot reach, x0 clipped).
 * Flat stretches of psi — the clamp at 0, the Box-Cox floor — contribute nothing to the integrals;
 * the atom they create is in F_X already.  The integrals run over [lo, hi], the range outside of
 * which every component's tail, times the growth of psi there, is below 1e-18,
 * split at x0 and at the boundaries of g, in uniform panels no wider than the smallest standard
 * deviation of the date, each with a Gauss-Kronrod 7/15 pair.
 *   w, mu, var      as ngp_mixture_crps
 *   inv             const void * to ONE ngp_inv_transform, as the path targets pass it
 *   scale, shift    shift >= 0, finite; ignored for NGP_SCORE_NATURAL
 *   y [m]           observations on the ORIGINAL scale
 *   tol             requested relative accuracy of crps; <= 0: the default, 1e-10
 *   crps [m]        CRPS(Y_j, yt_j) on the score scale (the K15 sums)
 *   mean [m]        E[Y_j] on the score scale; may be NULL
 *   err [m]         the call's own estimate of the absolute quadrature error of crps[j], the sum of
 *                   |K15 - G7| over the panels; may be NULL
 *   info [m]        0, or
 *                   c + 1: component c is bad at date j, as in the calls above (date NaN, other
 *                     dates untouched);
 *                   NGP_INFO_NOT_CONVERGED (-4): a date whose err exceeds tol |crps| is integrated
 *                     again at half the panel width, alone, up to 8,192 panels per date; at that
 *                     cap with err still above tol |crps| the values ARE returned, with this code;
 *                   NGP_INFO_NOT_FINITE (-3), date NaN: the score is infinite or psi is not
 *                     monotone where the mass is —
 *                       NGP_SCORE_LOG with shift = 0 (more precisely g + shift <= 0) on a stretch
 *                       that reaches into [lo, hi], i.e. positive mass where g = 0;
 *                       NGP_INV_BOXCOX with lam < 0 and more than 1e-12 of the date's mass beyond
 *                       the pole x = -1 / lam, where the reference's rule maps to 0 (mass within
 *                       that tolerance is ignored: the integral stops at the pole);
 *                       a result that is not finite in fp64 (exp overflow).
 * Accuracy: |crps - exact| <= err + 1e-13 sum_c w_c E|Y_c - yt| (the floor ngp_mixture_crps is
 * granted), and err <= tol |crps| whenever info = 0.  Identities:
 *   NGP_INV_IDENTITY + NATURAL                     = ngp_mixture_crps(y)
 *   NGP_INV_EXP (offset 0) + LOG (shift 0)         = ngp_mixture_crps(log y)
 *   one component, NGP_INV_EXP (offset 0) + NATURAL = the lognormal closed form (Baran & Lerch
 *     2015):  y (2 Phi(z) - 1) - 2 exp(mu + sd^2 / 2) (Phi(z - sd) + Phi(sd / sqrt 2) - 1),
 *     z = (ln y - mu) / sd
 * NGP_ERR_ARG, before anything touches a device: as ngp_mixture_crps, plus an unknown scale or
 * inv.kind; a non-finite shift, tol, lam, offset or cap; shift < 0; a non-finite y, or a y where
 * s(y) is undefined (y + shift <= 0 for NGP_SCORE_LOG).  Limits: those of ngp_mixture_crps.
 * Bitwise reproducible from call to call; a date's bits do not depend on the other dates of the
 * call (fixed-order sums, no floating-point atomics).  Thread-safe through the context's lock; not
 * combined with concurrent callers; not counted in ngp_profile.                                  */
enum { NGP_SCORE_NATURAL = 0, NGP_SCORE_LOG = 1 };
ngp_status ngp_mixture_crps_mapped(ngp_ctx *ctx, int32_t C, int32_t m, const double *w,
                                   const double *mu, const double *var, const void *inv,
                                   int32_t scale, double shift, const double *y, double tol,
                                   double *crps, double *mean, double *err, int32_t *info);

/* ---- cached factor ------------------------------
 * A fitted model is queried many times with the same particles and the same
 * training data: forecast() on several date grids, forecast_with_nowcasts()
 * after it (src/forecasting.jl:46, 135).  ngp_factor_create factorises the P
 * training covariances ONCE and keeps L (and the block inverses the solves
 * use) resident on the device; a query then only fills its aux rows (appended
 * points, forecast points, y) and sweeps them through L: O(n^2 (d + m)) per
 * particle instead of n^3 / 3.  Queries return exactly what
 * ngp_nowcast_batch returns for the same arguments (d = 0: plain predict).
 * The handle owns device memory of about 8 n (n + 192) bytes per particle;
 * it copies the kernels and the data it was created with.
 *   create : y is [P][n] with row stride ldy (0: one y shared by all)
 *   logml  : log p(y | particle) and the factorisation status of create
 *   nowcast: d + m <= NGP_MAX_AUX - (n mod 64) - 1                            */
typedef struct ngp_factor ngp_factor;
ngp_status ngp_factor_create(ngp_ctx *ctx, int32_t P, const ngp_kernel *kernels,
                             int32_t n, const double *t, const double *y, int64_t ldy,
                             ngp_factor **out);
ngp_status ngp_factor_logml(const ngp_factor *f, double *logml, int32_t *info);
ngp_status ngp_factor_nowcast(ngp_factor *f, int32_t d, const double *t_add,
                              int32_t D, const double *y_add,
                              int32_t m, const double *t_new, int32_t noise_on_new,
                              double *logml_base, double *logml_full,
                              double *mu, double *sigma, int32_t *info);
void       ngp_factor_destroy(ngp_factor *f);

/* ---- additive decomposition of a fitted model's forecast ------------------------
 * What AutoGP offers as `decompose`: which part of a forecast is trend, which is season.  A fitted
 * tree is almost always a sum.  Its COMPONENTS are the maximal non-Plus subtrees reached from the
 * root through Plus nodes only; in postfix order each is a contiguous slice of ops and of params,
 * so a component is itself a valid ngp_kernel.  A tree whose root is not Plus has one component,
 * itself.  ngp_kernel_components never splits a ChangePoint, nor a Plus below a Times or a
 * ChangePoint; ngp_kernel_terms below does (a ChangePoint's two summands ARE expressible in the
 * grammar: ChangePoint(k1, Constant(0)) and ChangePoint(Constant(0), k2)).
 *
 * For particle p with components c = 1..C, k = sum_c k_c, training times t,
 * K = k(t,t) + (noise + jitter) I, query dates t* (m of them) and X_c = k_c(t*, t):
 *     mu_c       = X_c K^-1 y                                         [m]
 *     Sigma_c,c' = delta_cc' k_c(t*, t*) - X_c K^-1 X_c'^T            [m x m]
 * the joint posterior of the independent latent parts g_c ~ GP(0, k_c) given y.  No noise term
 * appears: noise is a part of its own, the remainder y - sum_c g_c.  Against the noise-free
 * predict of the same factor (ngp_factor_nowcast with d = 0, noise_on_new = 0):
 *     sum_c mu_c = mu,   sum_c,c' Sigma_c,c' = Sigma,   every Sigma_c,c is positive semi-definite,
 * and the variance of any sum of components ("all seasonal parts") is the sum of its blocks.
 *
 * ngp_kernel_components (host only) does the slicing: component i of k is
 * ops[op_first[i] .. + op_len[i]), params[par_first[i] .. + par_len[i]), left to right.  The four
 * arrays hold up to NGP_MAX_OPS / 2 + 1 entries each and may be NULL (count alone).
 *
 * ngp_factor_components is ONE query of the resident factor: the C_p m component rows of a
 * particle share its aux block with the tail observations and the y row and are swept through the
 * resident L once; no m x n matrix crosses the bus.
 *   comp_count [P]       C_p >= 1
 *   comps      [sum C_p] component programs, particle-major.  The library does NOT check that
 *                        they sum to the particle's kernel: the formulas above are what it returns
 *                        for ANY k_c (K stays the factor's).  A component's `noise` is ignored.
 *   mu    [sum C_p][m]
 *   sigma per particle [C_p m][C_p m] row-major (row = c m + j), packed back to back; may be NULL
 *   var   [sum C_p][m]  the diagonals of sigma, bit for bit; may be NULL
 *   info  [P] as ngp_factor_logml, plus a pivot failure among the tail observations; may be NULL.
 *         An item with info > 0 returns NaN in all its outputs; other items are not affected.
 * Limit: (n mod 64) + 1 + C_p m <= NGP_MAX_AUX for every particle, else NGP_ERR_TOO_LARGE (longer
 * horizons: several calls on blocks of dates — covariances across blocks are then not formed).
 * Null arguments, m < 1 and C_p < 1 are NGP_ERR_ARG, a malformed component NGP_ERR_PROGRAM, all
 * before anything touches a device.  Runs under the factor's spec; thread-safe through the
 * context's lock like the other factor queries; not combined with concurrent callers.  Bitwise
 * reproducible from call to call (fixed summation order, no floating-point atomics).
 * Profile classes: the component fill is booked under 4, the component epilogue under 3.      */
ngp_status ngp_kernel_components(const ngp_kernel *k, int32_t *count, int32_t *op_first,
                                 int32_t *op_len, int32_t *par_first, int32_t *par_len);
ngp_status ngp_factor_components(ngp_factor *f, const int32_t *comp_count, const ngp_kernel *comps,
                                 int32_t m, const double *t_new, double *mu, double *sigma,
                                 double *var, int32_t *info);

/* ---- sum-of-products terms; the decomposition conditioned on nowcasts -------------
 * The trees real fits end in are ChangePoint / Times trees, whose root is no Plus.  The device
 * blend of a ChangePoint is  s(t1) a s(t2) + (1 - s(t1)) b (1 - s(t2))  in its operand values a, b
 * under BOTH cp_form values (the form only picks the sigmoid s), i.e. linear in a and in b, and a
 * Times distributes over a Plus.  The TERMS of a tree T are therefore kernels that sum to T:
 *     leaf                              {T}
 *     Plus(l, r)                        terms(l) then terms(r)
 *     ChangePoint(l, r; th)             {CP(x, Constant(0); th) : x in terms(l)} then
 *       with NGP_SPLIT_CHANGEPOINT      {CP(Constant(0), y; th) : y in terms(r)}
 *     Times(l, r) with NGP_SPLIT_TIMES  {Times(x, y)}, x in terms(l) outer, y in terms(r) inner
 * A ChangePoint / Times without its flag is one term, verbatim (a Plus below it is not split).
 * The transition of a ChangePoint itself is not split: each windowed term carries it.
 *
 * ngp_kernel_terms (host only) writes the terms as NEW programs back to back into ops_out /
 * params_out; term i is ops_out[op_first[i] .. + op_len[i]), params_out[par_first[i] .. +
 * par_len[i]).  *count is always the true number of terms.  NGP_ERR_TOO_LARGE (with *count set)
 * when count > max_terms, when a term does not pass ngp_kernel_check, or when ops_cap / par_cap /
 * a missing buffer cannot take the terms.  The number of terms, the longest term and the size of
 * all terms together are known from the tree's structure, so every one of these returns comes
 * before a term is built: what the call allocates is bounded by ops_cap and par_cap, however many
 * terms a product of sums asks for.  All six output arrays NULL: the count alone (no term is
 * built; a term longer than NGP_MAX_OPS / NGP_MAX_PARAMS is still reported).  A term never has
 * more ops or parameters than the tree.  split = 0 gives
 * exactly the programs ngp_kernel_components slices.  The tree may be longer than NGP_MAX_OPS
 * (up to 64 NGP_MAX_OPS) as long as its terms are not.
 *
 * ngp_factor_components_nowcast is ngp_factor_components conditioned on d appended points and D
 * scenarios of their values (ngp_factor_nowcast's t_add, y_add [D x d]): with t+ = [t; t_add],
 * y+_s = [y; y_add_s], K+ = k(t+, t+) + (noise + jitter) I, X_c = k_c(t*, t+)
 *     mu_c,s     = X_c (K+)^-1 y+_s                                    [m]
 *     Sigma_c,c' = delta_cc' k_c(t*, t*) - X_c (K+)^-1 X_c'^T          (the same for every scenario)
 * One query of the resident factor and one code path with ngp_factor_components: d = 0, D = 1
 * returns its bits.  Against ngp_factor_nowcast of the same arguments with noise_on_new = 0 the
 * means of a scenario add up to its mean, the blocks to sigma, and logml_full agrees.
 *   logml_full [P][D]           as ngp_factor_nowcast; may be NULL
 *   mu         [sum C_p][D][m]
 *   sigma, var, info            as ngp_factor_components; a pivot failure among the tail and the
 *                               appended points reports n0 + k (n0 = 64 floor(n / 64)), the item
 *                               is NaN in every output, logml_full included
 * Limit: (n mod 64) + d + 1 + C_p m <= NGP_MAX_AUX for every particle, else NGP_ERR_TOO_LARGE.
 * NGP_ERR_ARG as ngp_factor_components, and for d < 0, D < 1, null t_add / y_add with d > 0; all
 * before anything touches a device.  A scenario's outputs depend neither on D nor on its place
 * among the scenarios (fixed summation order, no floating-point atomics).  Runs under the factor's
 * spec and the context's lock; not combined with concurrent callers.  Profile classes 4 and 3.  */
enum { NGP_SPLIT_PLUS = 0, NGP_SPLIT_CHANGEPOINT = 1, NGP_SPLIT_TIMES = 2 };   /* flags, or-ed */
ngp_status ngp_kernel_terms(const ngp_kernel *k, int32_t split, int32_t max_terms, int32_t *count,
                            int32_t *op_first, int32_t *op_len, int32_t *par_first, int32_t *par_len,
                            int32_t *ops_out, int32_t ops_cap, double *params_out, int32_t par_cap);
ngp_status ngp_factor_components_nowcast(ngp_factor *f, int32_t d, const double *t_add, int32_t D,
                                         const double *y_add, const int32_t *comp_count,
                                         const ngp_kernel *comps, int32_t m, const double *t_new,
                                         double *logml_full, double *mu, double *sigma, double *var,
                                         int32_t *info);

/* ---- long horizons from the resident factor ---------------------------------------
 * ngp_factor_nowcast carries its dates as aux rows of the factorisation, so tail + d + m + 1 <=
 * NGP_MAX_AUX.  ngp_factor_predict_long does not: the dates (with the tail observations, the
 * appended points and y) are the right-hand-side panel of ONE blocked triangular solve against the
 * resident L (fp64 matrix cores), followed by the Schur algebra of the small conditioning block.
 * A daily grid over a year is one query.
 *   d, t_add, D, y_add, t_new, noise_on_new   exactly as ngp_factor_nowcast; d = 0 (D, t_add and
 *                                             y_add are then ignored) is plain predict
 *   mu    [P][max(D, 1)][m]   the layout of ngp_factor_nowcast's mu
 *   var   [P][m]              always written; the diagonal of sigma, bit for bit
 *   sigma [P][m][m]           may be NULL: no m x m object is then formed, on the device or on the
 *                             bus; mu and var have the same bits either way.  Exactly symmetric.
 *   info  [P]                 as ngp_factor_logml, plus a non-positive pivot among the tail and the
 *                             appended points (n0 + k, n0 = 64 floor(n / 64)); may be NULL.  An item
 *                             with info > 0 is NaN in all its outputs; other items are not affected.
 * For arguments both calls accept the result is ngp_factor_nowcast's, to rounding (same jitter and
 * noise conventions).  The weight update (logml_base / logml_full) is not part of this call:
 * ngp_factor_nowcast with m = 0 gives it.
 * Limits (NGP_ERR_TOO_LARGE, before anything touches a device): m <= NGP_MAX_LONG_HORIZON and
 * (n mod 64) + d + 1 <= NGP_MAX_AUX; then what the device memory holds for ONE particle — the
 * particles are worked through in chunks sized to the memory, a large P is never refused.
 * NGP_ERR_ARG: null f, t_new, mu or var; m < 1; d < 0; d > 0 with D < 1 or null t_add / y_add.
 * Runs under the factor's spec (always fp64); thread-safe through the context's lock like the
 * other factor queries; not combined with concurrent callers.  Bitwise reproducible from call to
 * call (fixed summation orders, no floating-point atomics).  Profile classes: the panel fill and
 * the small blocks are booked under 4, the solve under 6, the products of the solved rows under 2,
 * the conditioning block and the per-date algebra under 3.                                     */
#define NGP_MAX_LONG_HORIZON 4096
ngp_status ngp_factor_predict_long(ngp_factor *f, int32_t d, const double *t_add,
                                   int32_t D, const double *y_add,
                                   int32_t m, const double *t_new, int32_t noise_on_new,
                                   double *mu, double *var, double *sigma, int32_t *info);

/* ---- paths of a long horizon, drawn on the device -----------------------------------
 * ngp_factor_sample_long draws from the S mixtures whose components are the long query's: with
 * mu_p,s and sigma_p what ngp_factor_predict_long returns for the same d, t_add, D, y_add, m,
 * t_new and noise_on_new, `out` is what the contract of ngp_mixture_sample (shared components)
 * gives for (w, mu, sigma, draws, seed) — Philox4x32-10, counter (draw, scenario, block, 0), key =
 * seed; block 0 picks the component against the fp64 running sum of w[s] (strict <, fallback
 * P - 1); blocks 1 + j / 2 are Box-Muller pairs; x = mu_k,s + chol(sigma_k) z.  sigma never leaves
 * the device: it is factorised in place, 64 columns at a time, on the fp64 matrix cores, and the
 * paths are a triangular-matrix x panel product against normals staged once per path.
 *   w         [S][P]          S = d > 0 ? D : 1; rows sum to 1
 *   out       [S][draws][m]
 *   comp      [S][draws]      the component of every path; may be NULL
 *   mu        [P][S][m]       may be NULL; the bits ngp_factor_predict_long returns
 *   var       [P][m]          may be NULL; likewise
 *   info      [P]             may be NULL; as ngp_factor_predict_long
 *   chol_info [P]             may be NULL; first non-positive pivot of chol(sigma_p), 1-based; 0:
 *                             none.  A particle without weight in any scenario is not factorised
 *                             and reports 0, as does one whose info > 0 (its sigma is NaN).
 * A path picked from a particle with info > 0 or chol_info > 0 is NaN in every date; other paths
 * are not affected.  A path's bits depend on (seed, scenario, draw, its particle) alone: not on
 * `draws` (a call with fewer draws returns the first draws of a call with more), not on the paths
 * it shares a tile with, not on how the particles or the paths are chunked by the memory.  Fixed
 * summation orders, no floating-point atomics, bitwise reproducible from call to call.
 * NGP_ERR_ARG: null f, t_new, w or out; m < 1; draws < 1; d < 0; d > 0 with D < 1 or null t_add /
 * y_add.  NGP_ERR_TOO_LARGE: m > NGP_MAX_LONG_HORIZON, (n mod 64) + d + 1 > NGP_MAX_AUX,
 * S draws > INT32_MAX — all before anything touches a device —, then what the device memory holds
 * for the paths and ONE particle; a large P is never refused.  Runs under the factor's spec and
 * the context's lock; not combined with concurrent callers.  Profile classes: the long query's,
 * plus the pick, the grouping and the normals under 4, the factorisation of sigma under 1
 * (diagonal blocks) and 6 (the rows below them), the product under 2.                        */
ngp_status ngp_factor_sample_long(ngp_factor *f, int32_t d, const double *t_add,
                                  int32_t D, const double *y_add,
                                  int32_t m, const double *t_new, int32_t noise_on_new,
                                  const double *w, int32_t draws, uint64_t seed,
                                  double *out, int32_t *comp, double *mu, double *var,
                                  int32_t *info, int32_t *chol_info);

/* ---- paths of a long horizon from independent mixtures ------------------------------
 * ngp_factor_sample_long_indep is ngp_factor_sample_long for S mixtures that share no component
 * (refined scenario clones: every clone's particles have parameters, and data, of their own): the
 * factor's P items are S mixtures of P' = P / S components each, mixture-major — item s P' + k is
 * component k of mixture s.  There are no appended points: a clone holds its nowcast points as
 * data (ngp_factor_create with per-item y rows).  It is to ngp_factor_sample_long what
 * ngp_mixture_sample_indep is to ngp_mixture_sample.
 *   w         [S][P']         rows sum to 1
 *   seeds     [S]
 *   out       [S][draws][m]
 *   comp      [S][draws]      the component within the mixture, 0 .. P' - 1; may be NULL
 *   mu        [P][m]          may be NULL; the bits ngp_factor_predict_long returns for the same
 *                             factor and dates (d = 0)
 *   var       [P][m]          may be NULL; likewise
 *   info      [P]             may be NULL; as ngp_factor_predict_long
 *   chol_info [P]             may be NULL; as ngp_factor_sample_long.  An item with w = 0 is not
 *                             factorised and reports 0.
 * Same paths as the shared form, one mixture at a time: mixture s is keyed by seeds[s] with
 * scenario counter 0 — counter (draw, 0, block, 0) — and draws what ngp_factor_sample_long draws on
 * a factor created from that mixture's P' items alone with d = 0, w[s], `draws` and seed =
 * seeds[s], bit for bit; to rounding, what ngp_mixture_sample_indep draws from the long query's
 * moments.  One call replaces S factors and S calls.  The counters, the pick (fp64 running sum
 * over the mixture's own P' weights, strict <, fallback P' - 1) and the Box-Muller pairing are
 * those of ngp_mixture_sample.
 * A path's bits depend on (seeds[s], draw, its item) alone: not on `draws`, not on S, not on the
 * mixture's place in the call, not on the paths it shares a tile with, not on how the memory
 * chunks the items or the paths.  Fixed summation orders, no floating-point atomics, bitwise
 * reproducible from call to call.  A path picked from an item with info > 0 or chol_info > 0 is
 * NaN in every date; other paths, those of the same mixture included, are not affected.
 * NGP_ERR_ARG: null f, t_new, w, seeds or out; m < 1; draws < 1; S < 1; P not a multiple of S.
 * NGP_ERR_TOO_LARGE: m > NGP_MAX_LONG_HORIZON, (n mod 64) + 1 > NGP_MAX_AUX, S draws > INT32_MAX
 * — all before anything touches a device —, then what the device memory holds for the paths and
 * ONE item; a large P is never refused.  Runs under the factor's spec and the context's lock; not
 * combined with concurrent callers.  Profile classes: those of ngp_factor_sample_long.        */
ngp_status ngp_factor_sample_long_indep(ngp_factor *f, int32_t S,
                                        int32_t m, const double *t_new, int32_t noise_on_new,
                                        const double *w, int32_t draws, const uint64_t *seeds,
                                        double *out, int32_t *comp, double *mu, double *var,
                                        int32_t *info, int32_t *chol_info);

/* ---- the decomposition over a long horizon ------------------------------------------
 * ngp_factor_components_nowcast carries its C_p m component rows as aux rows, so (n mod 64) + d +
 * 1 + C_p m <= NGP_MAX_AUX: 42 dates per call at C_p = 3 with a tail of 63.
 * ngp_factor_components_long is the same decomposition (the same formulas, no noise term
 * anywhere) in the panel form of ngp_factor_predict_long: the panel of the ONE triangular solve
 * against the resident L holds, per particle, C_max groups of date rows, group c filled under the
 * particle's c-th component program.  A daily grid over a year is one query.
 *   d, t_add, D, y_add    as ngp_factor_predict_long; with d = 0, D, t_add and y_add are ignored;
 *                         S = d > 0 ? D : 1 scenarios
 *   comp_count, comps     as ngp_factor_components (not checked to sum to the kernel; a
 *                         component's `noise` is ignored)
 *   mu    [sum C_p][S][m] the layout of ngp_factor_components_nowcast
 *   cross per particle [C_p][C_p][m], packed back to back; always written.  cross[c][c'][j] =
 *         Sigma_c,c'[j, j], the covariance of parts c and c' at the SAME date: its c = c' planes are
 *         the variances, and the variance of any sum of parts at a date is the sum of its entries —
 *         C^2 m numbers where sigma has (C m)^2.  Exactly symmetric in (c, c').
 *   sigma per particle [C_p m][C_p m] (row = c m + j), packed back to back; may be NULL: no
 *         (C m)^2 object is then formed, on the device or on the bus; mu and cross have the same
 *         bits either way.  cross is its same-date diagonal bit for bit.  Exactly symmetric.
 *   info  [P] as ngp_factor_predict_long; may be NULL.  An item with info > 0 is NaN in all its
 *         outputs; other items are not affected.
 * Limits (NGP_ERR_TOO_LARGE, before anything touches a device): m <= NGP_MAX_LONG_HORIZON,
 * (n mod 64) + d + 1 <= NGP_MAX_AUX, and with sigma max_p C_p m <= NGP_MAX_LONG_HORIZON (also
 * C_p <= 65,534); then what the device memory holds for ONE particle — the particles are worked
 * through in chunks sized to the memory, a large P is never refused.
 * NGP_ERR_ARG: null f, comp_count, comps, t_new, mu or cross; m < 1; C_p < 1; d < 0; d > 0 with
 * D < 1 or null t_add / y_add.  NGP_ERR_PROGRAM: a malformed component.  All before device work.
 * Runs under the factor's spec and the context's lock; not combined with concurrent callers.
 * Bitwise reproducible from call to call (fixed summation orders, no floating-point atomics); a
 * particle's outputs depend neither on the other particles of the call nor on how the memory
 * chunks them.  Profile classes: those of ngp_factor_predict_long (fill and small blocks 4, solve
 * 6, products of rows 2, conditioning block and per-date algebra 3).                           */
ngp_status ngp_factor_components_long(ngp_factor *f, int32_t d, const double *t_add, int32_t D,
                                      const double *y_add, const int32_t *comp_count,
                                      const ngp_kernel *comps, int32_t m, const double *t_new,
                                      double *mu, double *cross, double *sigma, int32_t *info);

/* ---- hindcasts: the forecasts of one resident factor at many forecast origins ---------
 * What would this fitted model have forecast knowing only the first c observations?  The leading
 * c x c block of the resident Cholesky factor is the factor of the first c observations, so after
 * the ONE triangular solve of ngp_factor_predict_long every prefix of a date's solved panel row is
 * a forecast origin: the means and variances of R origins x m dates are running sums along the
 * rows (and on through the small conditioning block of the tail), not R factorisations.
 *   cut   [R]        strictly increasing, 1 <= cut <= n: origin r knows the first cut[r]
 *                    observations of the factor, in the order it was created with
 *   t_new [m], noise_on_new   as ngp_factor_predict_long (no appended points: d = 0)
 *   mu, var [P][R][m]  the predictive of the particle's GP conditioned on those observations alone;
 *                    the jitter and noise conventions of ngp_factor_predict_long
 *   logml [P][R]     log p(y_1:cut[r] | particle); may be NULL
 *   info  [P]        as ngp_factor_predict_long; may be NULL.  An item with info > 0 is NaN in all
 *                    its outputs; other items are not affected.
 * To rounding, origin r is ngp_factor_predict_long (d = 0) and ngp_factor_logml of a factor created
 * on the first cut[r] observations, and cut = n is this factor's own long query and logml (not bit
 * for bit: the running sums and the products on the matrix cores add in different orders).
 * Bitwise reproducible from call to call; an origin's outputs do not depend on which other origins
 * share the call, a particle's neither on the other particles nor on how the memory chunks them
 * (every sum runs k ascending, no floating-point atomics).
 * NGP_ERR_ARG: null f, cut, t_new, mu or var; R < 1; m < 1; a cut outside 1..n or not strictly
 * increasing.  NGP_ERR_TOO_LARGE: R > NGP_MAX_ORIGINS, m > NGP_MAX_LONG_HORIZON, (n mod 64) + 1 >
 * NGP_MAX_AUX; then what the device memory holds for ONE particle — a large P is never refused.
 * All before anything touches a device.  Runs under the factor's spec and the context's lock; not
 * combined with concurrent callers.  Profile classes: those of ngp_factor_predict_long, the passes
 * over the origins and the evidence under 3.                                                   */
#define NGP_MAX_ORIGINS 1024
ngp_status ngp_factor_predict_origins(ngp_factor *f, int32_t R, const int32_t *cut,
                                      int32_t m, const double *t_new, int32_t noise_on_new,
                                      double *mu, double *var, double *logml, int32_t *info);

/* ---- measurement hooks -----------------------------------------------------
 * HIP-event timing of the kernels a job launches, on the stream they are
 * launched on.  Classes: 0 = chol_col_glds_kernel (fat steps: trailing-update
 * GEMM + fused solve, the dominant kernel), 1 = chol_diag, 2 = gram,
 * 3 = epilogue, 4 = cov fill (and the other elementwise kernels around an evaluation: the lattice
 * tables, the leapfrog step of ngp_grad_job_hmc), 5 = K^-1 = W W' of a gradient job (grad_kinv*), 6 = chol_col_kernel (thin /
 * full steps, aux solves of a resident factor), 7 = aux_update_kernel,
 * 8 = diag_ahead_kernel (side stream, overlaps classes 1 and 6), 9 = the
 * mixed-precision fat steps (chol_col_glds_kernel<MIXED>), 10 = Gram refinement
 * of NGP_PREC_MIXED (backward sweep, covariance apply, small products), 11 = the
 * reverse-mode contraction of a gradient job (grad_alpha / grad_contract* / grad_reduce),
 * 12 = the fat steps of a gradient job's general leaf (chol_col_glds_kernel<.., IDENT>: aux
 * rows [I ; y'], the sweep that also produces W = L^-T) — a different instantiation from class 0,
 * with its own flops, bytes and rate (the Toeplitz leaf of a gradient job runs class 0),
 * 13 = chol_small_kernel: the whole factorisation of a short series (n0 <= 256) in one launch,
 * in place of classes 0, 1, 6, 8 and 12 (ngp_set_short_series_path). */
#define NGP_NUM_KERNEL_CLASSES 14
typedef struct ngp_profile {
    double   ms[NGP_NUM_KERNEL_CLASSES];       /* summed device time per class */
    int64_t  launches[NGP_NUM_KERNEL_CLASSES]; /* kernel launches per class    */
    double   flops[NGP_NUM_KERNEL_CLASSES];    /* algorithmic flops executed   */
    double   bytes[NGP_NUM_KERNEL_CLASSES];    /* algorithmic HBM bytes        */
} ngp_profile;
/* Lattice dates.  Dates that sit on a lattice t = tmin + q h (whole-day dates, before or after a
 * rescale to [0, 1]) let every job replace the transcendentals of stationary subtrees by tables of
 * k(q h); structured storage and the Toeplitz gradient path below build on the same decision.  It is
 * made per call from all dates of the call (t, t_add, t_new) and accepts a series only if
 *     max_ij |(t_i - t_j) - (q_i - q_j) h| <= 2.5 eps (tmax - tmin),
 * i.e. the table arguments are the date differences to rounding at the scale of the differences;
 * a lattice of more than 16 (dates) + 4096 steps is refused for the size of its tables.  Correctly
 * rounded lattice dates qualify when their origin lies within their span (max |t| <= tmax - tmin):
 * k / (n - 1), slope * (days - origin), whole-day numbers (exact).  Dates far from their origin —
 * decimal years 2020 + k / 52, 1e4 + u — carry eps |t| / 2 of representation noise each, many eps
 * of the span: they are NOT taken for a lattice and every covariance entry is evaluated from the
 * dates as given, which is correct to rounding for any dates, but slower.  A caller who wants the
 * table route subtracts the origin before the call. */
/* Storage option of staged fp64 value jobs (on by default).  On a regular series (the main
 * block's dates at a constant lattice stride) the covariance matrix of a stationary kernel tree is
 * Toeplitz, K_ik = f(|i - k|): 127 numbers describe a 64 x 64 tile exactly.  Such an item's tiles
 * below the block diagonal are then never written to HBM — the column sweep regenerates a tile
 * from those numbers in LDS where it would have read the stored tile.  The values are the table
 * entries the fill would have stored, so every result is bit-identical with the option off
 * (tests/test_structured_storage_gpu.py); off exists for that comparison and for A/B timing.
 * The same switch governs the Toeplitz gradient path of gradient jobs (ngp_logml_grad_batch,
 * ngp_grad_stage): on a regular series the items whose trees are stationary are evaluated from the
 * Cholesky factor alone — the diagonal sums of K^-1 that the gradient needs follow from its first
 * column (Gohberg-Semencul), n^3/3 flops instead of n^3.  That is other arithmetic, not other
 * storage: logml and gradients agree with the general path to rounding (1e-11 on gradients in the
 * tests), not bit for bit.  An item qualifies if its tree has no Linear / ChangePoint node and at
 * most 16 leaves, the series is regular (128 <= n <= 8192) and noise + jitter >= 1e-9 k(0) (the
 * formula loses about eps cond(K) digits; with the default jitter the guard never binds); which
 * qualifying items of a MIXED batch actually take it depends on the batch size unless
 * ngp_set_batch_invariant is on.  Applies to jobs staged after the call. */
ngp_status ngp_set_structured_storage(ngp_ctx *ctx, int32_t on);
/* Short series in one launch (on by default).  The column sweep is a chain of dependent launches
 * per 64-wide block column; at the reference's everyday size (a few hundred points, 24-64
 * particles: docs/vignettes/getting-started.jl:266-268) that chain is the whole call.  With this
 * option a job whose main block is at most 256 points (value jobs: n < 320; gradient jobs:
 * n <= 256) is factorised by ONE kernel, one workgroup per item, the matrix in registers as
 * 16 x 16 blocks; such jobs store every tile (no structured storage) and
 * their gradient items all take the general leaf.  The rule is the geometry's alone, so it does
 * not make an item's bits depend on its batch.  Results agree with the column sweep to rounding
 * (another summation order); off exists for that comparison and for A/B timing.  Resident factors
 * (ngp_factor_*) and mixed-precision jobs stay on the column sweep.  Applies to jobs staged after
 * the call. */
ngp_status ngp_set_short_series_path(ngp_ctx *ctx, int32_t on);

ngp_status ngp_profile_enable(ngp_ctx *ctx, int32_t on);
ngp_status ngp_profile_reset(ngp_ctx *ctx);
ngp_status ngp_profile_get(ngp_ctx *ctx, ngp_profile *out);

/* fp64 MFMA issue-rate microbenchmark (v_mfma_f64_16x16x4_f64); returns the
 * measured dense TFLOP/s over `iters` back-to-back MFMAs per wave.            */
ngp_status ngp_microbench_mfma_f64(ngp_ctx *ctx, int32_t iters, double *tflops);
/* Same loop with in-kernel stamps: out[0] TFLOP/s (wall), out[1] median shader cycles per MFMA
 * per wave, out[2] median shader clock held under load in GHz, out[3] waves per SIMD.      */
ngp_status ngp_microbench_mfma_f64_detail(ngp_ctx *ctx, int32_t iters, int32_t blocks_per_cu,
                                          double *out);
/* MFMA operand-map self test, all row-major: D[0:256] = A[16x4] B[4x16] through one
 * v_mfma_f64_16x16x4_f64; D[256:512] = the same product through four DPP-rotated
 * v_mfma_f64_4x4x4_4b_f64 gathered back to the 16x16x4 C/D layout (the k-loop fast path).
 * The caller compares both halves with A @ B.  D must hold 512 doubles.                 */
ngp_status ngp_selftest_mfma_layout(ngp_ctx *ctx, const double *A, const double *B, double *D);
/* The same for the fp32 form of the mixed-precision path: D[32x32] = A[32x2] B[2x32] through one
 * v_mfma_f32_32x32x2_f32 (all row-major floats).                                          */
ngp_status ngp_selftest_mfma_f32_layout(ngp_ctx *ctx, const float *A, const float *B, float *D);
/* Pair terms A(mu_c - mu_c', var_c + var_c') per second with the operands in registers (no loads):
 * the ceiling the CRPS cross-term kernel is measured against; `iters` terms per thread.         */
ngp_status ngp_microbench_mixture_pairs(ngp_ctx *ctx, int32_t iters, double *pairs_per_s);
/* HBM streaming-write microbenchmark (GB/s) used to anchor the fill roofline. */
ngp_status ngp_microbench_hbm(ngp_ctx *ctx, int64_t bytes, double *write_gbs, double *copy_gbs);

#ifdef __cplusplus
}
#endif
#endif /* NGP_H */

// ngp_internal.h — shared between the kernel TU (ngp_kernels.hip) and the host/C-ABI TU
// (ngp_api.hip).  gfx950 only; no portability layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/ngp.h"

namespace ngp {

constexpr int NB = 64;        // block-column width of the left-looking factorisation
constexpr int TB = 16;        // MFMA tile edge (v_mfma_f64_16x16x4_f64)
constexpr int DEV_STACK = 8;  // register-resident evaluation stack depth on the device
constexpr int SPLITK_SLOTS = 16;   // (tile pair, piece) slots per item in ChunkPtrs::splitk_part

// device opcode = host opcode, plus CP with its two operands in swapped stack order
// (the host reorders children so the evaluation stack never exceeds DEV_STACK)
constexpr int OP_CP_SWAPPED = 9;
// reduced program only: a whole stationary subtree (no Linear, no ChangePoint below it) read from
// its table by lattice distance
constexpr int OP_TABLE = 10;
constexpr int RLEAF_TABLE = 1, RLEAF_LINEAR = 2;   // DevProgram::rops >> 4
constexpr int MAX_TABLES = NGP_MAX_OPS / 2;   // a tree of NGP_MAX_OPS nodes has at most that many leaves

// One particle's kernel, flattened for the device.  Copied into LDS by every workgroup that
// needs it; ops are uniform across the workgroup so the interpreter never diverges.
struct DevProgram {
    int32_t n_ops;
    int32_t n_params;
    double  noise;               // observation-noise variance (jitter is in the spec)
    uint8_t ops[NGP_MAX_OPS];
    uint8_t slot[NGP_MAX_OPS];   // per op: table slot (stationary leaf) or sigmoid slot (ChangePoint)
    uint8_t first[NGP_MAX_OPS];  // binary ops: index of the operand evaluated first (the second is i-1)
    uint8_t poff[NGP_MAX_OPS];   // per op: offset of its parameters in params[]
    double  params[NGP_MAX_PARAMS];
    // Reduced program for value jobs on lattice times: every maximal stationary subtree is ONE
    // table leaf (its value depends on |t1 - t2| only, so tables_kernel evaluates the subtree once
    // per lattice distance — the same operations in the same order as element by element).
    // A binary operation whose second operand is a leaf carries that leaf with it (high nibble of
    // rops: RLEAF_TABLE / RLEAF_LINEAR, rleaf = its table slot / parameter offset): the operation
    // then works on the top of the stack in place — a left-deep tree never moves the stack at all.
    // Same operands, same operation: the value is bit-identical to the unfused evaluation.
    int32_t n_rops, n_tab;
    int32_t rchain, rpad_;              // rchain: the reduced program pushes once (its first
                                        // instruction) and every other instruction carries its leaf
    uint8_t rops[NGP_MAX_OPS];          // low nibble: NGP_OP_LINEAR, OP_TABLE, Plus / Times / ChangePoint (+ swapped)
    uint8_t rslot[NGP_MAX_OPS];         // OP_TABLE: table slot; ChangePoint: sigmoid slot (= slot[] of the op)
    uint8_t rpoff[NGP_MAX_OPS];         // Linear / ChangePoint: offset of the parameters
    uint8_t rleaf[NGP_MAX_OPS];         // fused leaf: table slot (RLEAF_TABLE) or parameter offset (RLEAF_LINEAR)
    uint8_t tb_first[MAX_TABLES];       // table k tabulates ops[tb_first[k] .. tb_last[k]] (a postfix
    uint8_t tb_last[MAX_TABLES];        //  range of the full program = one subtree)
};
static_assert(sizeof(DevProgram) % 8 == 0, "DevProgram is copied as 8-byte words");
// the whole tree is stationary: its reduced program is ONE table lookup (fill_single_kernel)
__host__ __device__ inline bool prog_single_table(const DevProgram *P) {
    return P->n_rops == 1 && P->rops[0] == OP_TABLE;
}
// Structured items (JobGeom::toep: their tiles below the block diagonal are never stored, the
// column kernels regenerate them from 127 numbers in LDS):
//   1  the whole tree is stationary        K_ik = tab[toep |i - k|]            (Toeplitz)
//   0  anything else: stored
// (A single Linear leaf, K_ik = bias + amp (t_i - c)(t_k - c), was built as a second kind — 17 % of
// the bench ensemble, fill 35 -> 29 ms — and taken out again: with a second kind in the epilogue
// the fat kernel, stored tiles included, ran 4-5 % slower, whichever way the two kinds shared the
// code; profiles/r03/README.md.)
__host__ __device__ inline int prog_structure(const DevProgram *P) {
    return (P->n_rops == 1 && P->rops[0] == OP_TABLE) ? 1 : 0;
}
struct DevSpec {
    int32_t se_form, periodic_form, cp_form, precision;
    double  jitter;
    double  mixed_tau;   // NGP_PREC_MIXED: see ngp_spec in include/ngp.h
};

// Geometry of one staged job on the device (all items share times; see ngp_api.hip).
struct JobGeom {
    int32_t B;         // items (kernels)
    int32_t n0;        // main block: multiple of NB training points
    int32_t nb0;       // n0 / NB
    int32_t da;        // appended rows: tail (n - n0) + d nowcast points
    int32_t tail;      // n - n0: appended rows that belong to the base data
    int32_t m;         // forecast points
    int32_t naux;      // da + m + 1 (last aux row carries y)
    int32_t naux_pad;  // naux rounded up to a multiple of NB
    int32_t D;         // scenarios
    int32_t d;         // nowcast points per scenario
    int32_t noise_on_new;
    int32_t y_shared;  // 1: one base y / ya for all items
    int32_t lattice;   // 1: all times sit on a lattice t = tmin + q h  -> table-driven fill
    int32_t R;         // lattice table length (max |q_i - q_j| + 1)
    int32_t npts;      // n0 + da + m points that carry a time
    int32_t maxstat;   // stationary-leaf table slots per item
    int32_t maxcp;     // ChangePoint sigmoid slots per item
    int32_t n_real;    // main-block points that are data; rows/cols beyond are identity padding
    int32_t aux_identity;  // 1: aux rows are [I_n0 ; y'] (gradient path: W = L^-T)
    int32_t maxops;    // longest program of the batch (gradient jobs: picks the contraction kernel)
    int32_t aux_e1;    // 1: the Toeplitz gradient path — aux rows [y' ; e_1'] (the row after y' is e_1')
    int32_t toep;      // > 0: the main-block points sit on the lattice at a constant stride (q_i = q_0
                       // +- toep i), so K of a stationary tree is Toeplitz: K_ik = tab[toep |i - k|].  The
                       // fill then writes only the diagonal tiles and the aux rows of structured items
                       // (prog_structure) and the column kernels regenerate a tile from 128 numbers in
                       // LDS where they would have read the stored tile (staged fp64 value jobs; else 0)
    int32_t tab_sub;   // gradient jobs: table slot of the first SUBTREE table (the reduced program's tables
                       // follow the per-leaf ones, maxstat counts both); value jobs: 0
    int32_t invariant; // ngp_set_batch_invariant: nothing about an item's arithmetic may depend on
                       // the size of the batch it travels in (no split-k of small chunks, gradient
                       // routing and contraction shapes by item / geometry only, the epilogue never
                       // on the resident tables of a single-chunk job)
    int32_t short_series;  // ngp_set_short_series_path: n0 <= 256 is factorised in one launch
    int32_t pad_;
    double  h;         // lattice step
    int64_t ld;        // row stride of the factor storage (= n0)
    int64_t item_stride;  // elements per item in the factor storage
};

struct ChunkPtrs {
    double       *L;      // [Bc][(n0 + naux_pad) x n0] factor + aux rows, row-major
    double       *dinv;   // [Bc][64 strips x 64 lanes] L_jj^-1 of the current step, MFMA strip order
    const DevProgram *progs;  // [Bc] (already offset to the chunk)
    const DevProgram *progs_src;  // resident gradient jobs with new parameters: the programs in page-locked
                              // HOST memory — tables_kernel reads them from there and leaves the device copy
                              // (progs) for the kernels behind it, instead of a copy ahead of the chain; else null
    const double *t0;     // [n0]
    const double *taux;   // [da + m] times of the aux rows (appended then forecast)
    const double *y0;     // [Bc or 1][n0] (already offset to the chunk when per item)
    double       *logdet; // [Bc]
    int32_t      *info;   // [Bc]
    double       *tab;    // [Bc][maxstat][R]   stationary-leaf values by lattice distance
    double       *sig;    // [Bc][maxcp][npts]  ChangePoint sigmoids by point
    const int32_t *qpts;  // [npts] lattice coordinate of every point (t0 then taux)
    double       *dtab;   // [Bc][maxstat][3][R] gradient jobs on a lattice: per stationary leaf the
                          // unscaled factor e and the two parameter-derivative factors (else null)
    // ---- NGP_PREC_MIXED jobs only (all null otherwise) ----
    float        *L32;    // [Bc][item_stride] fp32 shadow of the finished off-diagonal tiles of L
                          // and of the aux rows W (operands of the fp32 tile products)
    float        *tmax;   // [Bc][nb0 + naux_pad/64][nb0] max |.| of every finished 64x64 tile
                          // (row tile, block column); aux tiles follow the nb0 main row tiles
    unsigned     *mixcnt; // [Bc][2] tile products of the fat steps that ran in fp32 / in fp64
    double       *auxX;   // [Bc][naux_pad][n0] the fill also leaves the aux rows X here
    const int32_t *order; // mixed fat steps: dispatch order of the items (heaviest first) or null
    // staged value jobs on a lattice: the chunk's items split by the shape of their reduced program
    // (job-wide indices, ascending; item of the chunk = entry - fill_base); null: every item goes
    // through the general fill
    const int32_t *fill_chain, *fill_other, *fill_single;
    int32_t n_fill_chain, n_fill_other, n_fill_single, fill_base;
    double       *G;      // short value jobs: [Bc][naux x naux] — chol_small_kernel leaves the Gram matrix
                          // of the aux rows itself (gram_kernel's arithmetic, one launch less); else null
    const int32_t *items; // refinement sweeps: the items (indices into the chunk) a launch works
                          // on, Bc = their count; null: all of them in order
    // small chunks only (null otherwise): split-k fat steps, see chol_col_glds_kernel<.., SPLITK>
    double       *splitk_part;  // [Bc][SPLITK_SLOTS][4 waves][64 x 64] accumulator tiles of the pieces
};

struct EpiPtrs {
    const DevProgram *progs;  // [B]
    const double *taux;       // [da + m]
    const double *G;          // [B][naux x naux]
    const double *ya;         // [B or 1][D][da]
    const double *logdet;     // [B]
    int32_t      *info;       // [B]
    double       *work;       // [B][work_stride]
    double       *zbuf;       // [B][D][da]
    double       *logml_base; // [B]
    double       *logml_full; // [B][D]
    double       *mu;         // [B][D][m]
    double       *sigma;      // [B][m][m]
    int64_t       work_stride;
    // lattice tables of the aux points when they are still resident (single-chunk jobs), else null:
    // the small Schur blocks are then lookups instead of fp64 transcendental evaluations
    const double *tab, *sig;  // [B][maxstat][R], [B][maxcp][npts]
    const int32_t *qpts;      // [npts]
};

// ngp_factor_components (ngp_component_kernels.h): the forecast rows of the query are Cmax groups of
// m dates, group c of an item evaluated under the item's c-th component program
struct CompPtrs {
    const DevProgram *progs;  // [sum C_b] component programs, item-major
    const int32_t *first;     // [B + 1] an item's first component (running sum of C_b)
    const int64_t *sig_off;   // [B] where the item's [C_b m][C_b m] block starts in sigma
    double       *mu;         // [sum C_b][D][m]
    double       *sigma;      // the items' blocks back to back, or null
    double       *var;        // [sum C_b][m], or null
    int32_t       m;          // dates per component
    int32_t       cmax;       // max C_b: the geometry's m is cmax * m
};

// ngp_factor_predict_long (ngp_long_kernels.h): the dates are the panel of a triangular solve
// against the resident L, not aux rows of the factorisation
constexpr int LONG_TILE = 64;          // panel columns a wave owns in the solve
constexpr int LONG_WG_TILE = 256;      // panel columns of a workgroup: block row j of L is read once per such tile
struct LongGeom {
    int32_t B;             // items of the chunk
    int32_t n0, nb0;       // the resident main block
    int32_t c;             // conditioning points: tail (n - n0) + d appended
    int32_t m, D;          // dates, scenarios
    int32_t q1;            // panel rows: y', the c conditioning points, the m dates
    int32_t qpad;          // q1 rounded up to a multiple of LONG_TILE
    int32_t noise_on_new, y_shared, want_sigma, pad_;
    int64_t ld;            // row stride of L and of the panel (= n0)
    int64_t L_stride;      // elements per item in the factor storage
    int64_t dinv_step;     // elements between the block inverses of consecutive block columns
    int64_t sig_ld;        // row stride of an item's sigma (m; ngp_factor_sample_long: m rounded up to NB)
    int64_t sig_stride;    // elements per item in sigma
};
struct LongPtrs {
    const DevProgram *progs;   // [B]
    const double *L;           // the chunk's first item in the resident factor
    const double *dinv;        // block column 0, the chunk's first item
    const int32_t *finfo;      // [B] the factor's status of create; null without a main block
    const double *t0;          // [n0]
    const double *tp;          // [c + m] tail, appended points, dates
    const double *y0;          // [B or 1][n0]
    const double *yc;          // [B or 1][D][c]
    double *W;                 // [B][qpad][n0]
    double *S;                 // [B][q1][c + 1]
    double *dg;                // [B][q1]
    double *z;                 // [B][D][c]
    double *mu, *var, *sigma;  // [B][D][m], [B][m], [B][m][m] or null
    int32_t *info;             // [B]
};
// step: 0 fill, 1 small blocks, 2 solve, 3 products of the rows, 4 conditioning block, 5 dates, 6 sigma
enum { LONG_FILL = 0, LONG_SMALL, LONG_SOLVE, LONG_GRAM, LONG_COND, LONG_APPLY, LONG_SIGMA };
void launch_long(int step, const LongGeom &g, const LongPtrs &p, const DevSpec &sp, hipStream_t s);

// ngp_factor_components_long (ngp_long_component_kernels.h): the long query's panel with the m date
// rows replaced by cmax groups of date rows, group c of an item filled under its c-th component
// program.  The LongGeom of the call has q1 = qpad = hpad + cmax mpad (every panel row is a row of S
// too), LongPtrs::tp holds the conditioning points and the m dates once, dg / mu / var / sigma of
// LongPtrs stay null.
struct LongCompGeom {
    int32_t m, mpad;       // dates per component; m rounded up to LONG_TILE: the rows of a group
    int32_t cmax;          // groups of the panel: the call's largest C_p
    int32_t hpad;          // y' and the c conditioning rows, rounded up to LONG_TILE: group c starts
                           // at row hpad + c mpad, so date i of every group sits at the same place of
                           // its 64-row tile
};
struct LongCompPtrs {
    const DevProgram *progs;   // the component programs of the chunk's first item onward
    // running sums over the particles of the CALL, entry 0 = the chunk's first item: an item's place
    // in the chunk's outputs is its entry minus entry 0
    const int32_t *first;      // [B + 1] C_b
    const int64_t *cr_off;     // [B + 1] C_b^2
    const int64_t *sig_off;    // [B + 1] (C_b m)^2
    double *mu;                // [sum C_b][D][m]
    double *cross;             // per item [C_b][C_b][m]
    double *sigma;             // per item [C_b m][C_b m], or null
};
// step: 0 fill, 1 small blocks, 2 products of the rows, 3 means, 4 cross, 5 sigma; the solve and the
// conditioning block are launch_long's
enum { LCOMP_FILL = 0, LCOMP_SMALL, LCOMP_GRAM, LCOMP_APPLY, LCOMP_CROSS, LCOMP_SIGMA };
void launch_long_comp(int step, const LongGeom &g, const LongPtrs &p, const LongCompGeom &cg,
                      const LongCompPtrs &cp, const DevSpec &sp, hipStream_t s);

// ngp_factor_predict_origins (ngp_long_origin_kernels.h): the long query without appended points,
// read at R prefixes of the observations.  LongPtrs::mu / var / sigma stay null.
struct LongOriginGeom {
    int32_t R;             // origins
    int32_t R0;            // of them inside the main block (cut <= n0): the cuts are sorted
};
struct LongOriginPtrs {
    const int32_t *cut;    // [R] strictly increasing, 1 .. n
    double *mu, *var;      // [B][R][m]
    double *logml;         // [B][R], or null
};
// step: 0 origins inside the main block (between the solve and the products of the rows), 1 origins
// in the conditioning block, 2 evidence (both behind the conditioning block)
enum { LORG_MAIN = 0, LORG_TAIL, LORG_LOGML };
void launch_long_origin(int step, const LongGeom &g, const LongPtrs &p, const LongOriginGeom &og,
                        const LongOriginPtrs &op, const DevSpec &sp, hipStream_t s);

// ngp_factor_sample_long (ngp_long_sample_kernels.h): paths of a long horizon from the sigma the
// long query leaves on the device.  sigma is stored [mpad x mpad] per item (mpad: m rounded up to
// NB, the padding a unit diagonal), factorised in place 64 columns at a time, and the paths of a
// particle are a lower-triangular x panel product against their staged normals.
constexpr int LS_THREADS = 256;
constexpr int LS_WG_PATHS = 256;       // paths of a workgroup of the product: four waves, 64 each
struct LongSampleGeom {
    int32_t P, S, draws, m;
    int32_t mpad, nb;      // m rounded up to NB; mpad / NB
    int32_t mu_rows;       // rows of mu per item: S, or 1 where every item has its own mean alone
    int32_t mu_own;        // 1: a path adds row s of its item's means; 0: the item's one row
    int64_t N;             // S draws
    int64_t stride;        // elements per item in sigma: mpad mpad
};
struct LongSamplePtrs {
    double *sigma;             // [B][mpad][mpad] the run's first item: sigma in, L out
    double *dinv;              // [B][NB NB] inverse of the current diagonal block, MFMA strip order
    double *logdet;            // [B] scratch of the diagonal step
    int32_t *cinfo;            // [B] first non-positive pivot, 1-based; 0: none
    const int32_t *info;       // [B] the long query's status
    const double *mu;          // [B][mu_rows][m]
    const uint32_t *off;       // [B + 1] first sorted position of each item's paths
    const int32_t *order;      // [N] path (s draws + d) at each sorted position
    const double *Z;           // [zrows + NB][mpad] normals of sorted positions zfirst ..
    double *out;               // [N][m]
};
// pick: comp [N].  count: cnt [P].  group: order [N] from off [P + 1] (ascending path inside a group)
void launch_ls_pick(const LongSampleGeom &g, const double *w, uint64_t seed, int32_t *comp, hipStream_t s);
void launch_ls_count(const LongSampleGeom &g, const int32_t *comp, uint32_t *cnt, hipStream_t s);
void launch_ls_group(const LongSampleGeom &g, const int32_t *comp, const uint32_t *off, int32_t *order,
                     hipStream_t s);
void launch_ls_normals(const LongSampleGeom &g, uint64_t seed, const int32_t *order, int64_t zfirst,
                       int64_t zrows, double *Z, hipStream_t s);
void launch_ls_pad(const LongSampleGeom &g, double *sigma, int B, hipStream_t s);
// block column j of B items: the diagonal block (and its inverse), then the row blocks below it
void launch_ls_diag(const LongSampleGeom &g, const LongSamplePtrs &p, int B, int j, hipStream_t s);
void launch_ls_panel(const LongSampleGeom &g, const LongSamplePtrs &p, int B, int j, hipStream_t s);
// paths of sorted positions [zfirst, zfirst + zrows) that belong to the B items; tiles: the
// largest number of LS_WG_PATHS groups any of them needs
void launch_ls_draw(const LongSampleGeom &g, const LongSamplePtrs &p, int B, int64_t zfirst, int64_t zrows,
                    int tiles, hipStream_t s);
// ngp_factor_sample_long_indep (ngp_long_sample_indep_kernels.h): the geometry's P items are S
// mixtures of Pm components each, mixture-major, mixture s keyed by seeds[s].  pick: item [N] (the
// item s Pm + k, what count and group sort by) and comp [N] (k).  normals: as launch_ls_normals
void launch_lsi_pick(const LongSampleGeom &g, int Pm, const double *w, const uint64_t *seeds, int32_t *item,
                     int32_t *comp, hipStream_t s);
void launch_lsi_normals(const LongSampleGeom &g, const uint64_t *seeds, const int32_t *order, int64_t zfirst,
                        int64_t zrows, double *Z, hipStream_t s);

// ---- short series in one launch (ngp_small_kernels.h) ------------------------------------
constexpr int SM_WAVES = 8, SM_THREADS = 64 * SM_WAVES;   // two waves per SIMD: 256 VGPRs each
constexpr int SM_NSLOT = 20;           // register blocks per wave (8 VGPRs each)
constexpr int SM_DSTR = 17;            // row stride of a diagonal block in LDS (doubles)
constexpr int SM_MAX_PANEL = 34;       // panel blocks of one step: main rows + the sweep's aux row-blocks
constexpr int SM_MAX_SWEEPS = 4;

// One sweep over the block columns.  Aux row-blocks taken along: identity rows [i0, i1) (gradient
// jobs: row-block a is e_(16a..16a+15)', it joins at column a and stays upper triangular) and dense
// rows [a0, a1) (slab rows n0 + 16 a ...).
struct SmallSweep {
    int32_t main;          // 1: factorise the main block; 0: aux rows only, against the stored factor;
                           // 2: the inverse phase of a gradient job — W_I = L^-T block column by block
                           // column of L^-1, every column a wave's own task (SmallPlan::colwave)
    int32_t i0, i1, a0, a1;
};
struct SmallPlan {
    int32_t nbe;           // 16-blocks of the main block that hold data: ceil(n_real / 16)
    int32_t nsweeps;
    int32_t ident;         // gradient job (aux rows [I ; y'])
    int32_t npanel;        // panel blocks to reserve in LDS
    uint64_t colwave;      // inverse phase: 4 bits per block column j — the wave that computes it
    SmallSweep sw[SM_MAX_SWEEPS];
};

constexpr int SM_LDS_FIXED = 8 * (16 * 256 + 16 * 16 * SM_DSTR + 256 + 32);   // M_j | diagonal blocks | pivots | flags
inline int small_lds_bytes(const SmallPlan &pl) { return SM_LDS_FIXED + pl.npanel * 2048; }

enum { COL_FULL = 0, COL_FAT = 1, COL_THIN = 2, COL_AUX = 3 };   // launch_chol_col's mode

}  // namespace ngp
// the route rules (small_plan, small_job, the column schedule, every threshold) and the roofline
// accounting of the launches: host-only headers over the structs above
#include "ngp_plan.h"
#include "ngp_cost.h"
#include "ngp_mixmap_plan.h"
namespace ngp {

void launch_chol_small(const JobGeom &g, const ChunkPtrs &p, int Bc, const SmallPlan &pl, hipStream_t s);
// K^-1 = W_I W_I', alpha = W_I z and z'z of a short gradient job in one launch (16 x 16 blocks)
void launch_grad_kinv_small(const JobGeom &g, const double *L, double *Kinv, double *alpha, double *quad,
                            int Bc, hipStream_t s);

// ---- launchers implemented in ngp_kernels.hip ------------------------------------------
void launch_tables(const JobGeom &g, const ChunkPtrs &p, int Bc, const DevSpec &sp, hipStream_t s);
void launch_fill(const JobGeom &g, const ChunkPtrs &p, int Bc, const DevSpec &sp, hipStream_t s,
                 bool aux_only = false);
void launch_chol_diag(const JobGeom &g, const ChunkPtrs &p, int Bc, int j, int k0, hipStream_t s);
// sp: only mixed_tau / jitter are read, and only when p.L32 is set (mixed-precision job)
void launch_chol_col(const JobGeom &g, const ChunkPtrs &p, int Bc, int j, int mode, int k0,
                     hipStream_t s, const DevSpec *sp = nullptr);
// ---- Gram refinement of NGP_PREC_MIXED (G = X K^-1 X' against the fp64 covariance) ----
// A_c = C_c L_cc^-1, then C_j -= A_c L_(c,j) for j < c, c descending: C (aux rows of the slab,
// [Bc][naux_pad][n0] at rows n0.. of p.L) becomes C (L L')^-1 ... see aux_back_kernel
void launch_aux_back(const JobGeom &g, const ChunkPtrs &p, const double *dinv_all, size_t mstep,
                     double *Aout, int accumulate, int Bc, int c, hipStream_t s);
// R = X - A K  (K re-evaluated tile by tile from the kernel trees / lattice tables)
void launch_kapply(const JobGeom &g, const ChunkPtrs &p, const double *A, const double *X,
                   double *R, int Bc, const DevSpec &sp, hipStream_t s);
// G = sym(A X' + R A'); delta[2b] = max |R A'| relative to sqrt(G_aa G_bb), delta[2b+1] = max_a |R_a|/|X_a|
void launch_refine_gram(const JobGeom &g, const double *A, const double *X, const double *R,
                        double *S, double *T, double *U, double *G, double *delta, int Bc,
                        const int32_t *items, hipStream_t s);
void launch_mfma_f32_probe(const float *A, const float *Bm, float *Dout, hipStream_t s);
void launch_diag_ahead(const JobGeom &g, const ChunkPtrs &p, int Bc, int j, hipStream_t s);
// order <- items by fp64 tile products since the last call, most first (prev: [Bc] snapshot)
constexpr int NGP_MIXED_ORDER_MAX = 8192;   // items mixed_order_kernel ranks in LDS (32 KiB)
bool launch_mixed_order(const ChunkPtrs &p, unsigned *prev, int32_t *order, int Bc, hipStream_t s);
void launch_aux_update(const JobGeom &g, const ChunkPtrs &p, int Bc, int j, hipStream_t s);
// side / fork / join: when given, alpha is computed beside K^-1 on the side stream
void launch_grad_kinv(const JobGeom &g, const double *L, double *Kinv, double *alpha, double *quad,
                      int Bc, hipStream_t s, hipStream_t side = nullptr, hipEvent_t fork = nullptr,
                      hipEvent_t join = nullptr);
// items / bucket_counts: the chunk's items (chunk-local indices) sorted by tree size into
// GRAD_BUCKETS groups (grad_bucket, ngp_plan.h) — at most 1, 2, 4, 8, 16 leaves, larger — and the size of every group;
// null: one launch for the whole chunk, sized by g.maxops
void launch_grad_contract(const JobGeom &g, const ChunkPtrs &p, const double *Kinv,
                          const double *alpha, const double *quad, double *partials, double *grad,
                          double *logml, int Bc, const DevSpec &sp, hipStream_t s,
                          const int32_t *items = nullptr, const int32_t *bucket_counts = nullptr,
                          hipStream_t side = nullptr, hipEvent_t fork = nullptr,
                          hipEvent_t join = nullptr);
void launch_toep_grad(const JobGeom &g, const ChunkPtrs &p, const double *A, double *wbuf,
                      const double *quad, double *partials, double *grad, double *logml, int Bc,
                      const DevSpec &sp, hipStream_t s, const int32_t *items = nullptr,
                      const int32_t *bucket_counts = nullptr);
void launch_toep_quad(const JobGeom &g, const double *L, double *quad, int Bc, hipStream_t s);
void launch_gram(const JobGeom &g, const double *L, double *G, int Bc, hipStream_t s);
void launch_epilogue(const JobGeom &g, const EpiPtrs &p, const DevSpec &sp, hipStream_t s);
// component rows of a resident factor's query: their fill (behind launch_fill(.., aux_only), which
// leaves the tail and y' rows) and the epilogue that stands in for launch_epilogue
// component_epilogue_kernel keeps L_A [da x da] and four vectors of da in dynamic LDS while they
// fit COMP_EPI_LDS_BYTES (da <= 76), else behind V in the per-item work buffer
constexpr int COMP_EPI_LDS_BYTES = 48 * 1024;
inline int64_t comp_epi_small(int da) { return (int64_t)da * da + 4 * (int64_t)da; }   // doubles
void launch_component_fill(const JobGeom &g, const ChunkPtrs &p, const CompPtrs &cp, int Bc,
                           const DevSpec &sp, hipStream_t s);
void launch_component_epilogue(const JobGeom &g, const EpiPtrs &p, const CompPtrs &cp,
                               const DevSpec &sp, hipStream_t s);
void launch_cov(const DevProgram *progs, int B, const double *t1, int n1, const double *t2,
                int n2, int add_diag, double *out, const DevSpec &sp, hipStream_t s);
void launch_mixture_sample(int P, int S, int m, const double *w, const double *mu, double *chol,
                           int draws, uint64_t seed, const uint64_t *seeds, double *out,
                           int32_t *comp, int32_t *info, hipStream_t s);
// ---- summaries of a mixture's per-date marginals (ngp_mixture_kernels.h) -------------------
// w [C], mu / var / inv [m][C] date-major (inv = 1 / sqrt(2 var), launch_mixture_prep); the cross
// term of the CRPS is cut into MIX_TILE x MIX_TILE tiles of the upper triangle, one partial each
// in slab [m][mix_tile_pairs(C)]
constexpr int MIX_TILE = 256;
constexpr int MIX_MAX_COMPONENTS = 65536, MIX_MAX_POINTS = 4096, MIX_MAX_DATES = 65535;
inline int mix_tiles(int C) { return (C + MIX_TILE - 1) / MIX_TILE; }
inline int64_t mix_tile_pairs(int C) { const int64_t nt = mix_tiles(C); return nt * (nt + 1) / 2; }
void launch_mixture_prep(const double *var, double *inv, int64_t n, hipStream_t s);
void launch_mixture_cdf(int C, int m, const double *w, const double *mu, const double *inv, int K,
                        const double *x, double *out, hipStream_t s);
void launch_mixture_quantiles(int C, int m, const double *w, const double *mu, const double *inv,
                              int Q, const double *probs, double *q, hipStream_t s);
void launch_mixture_crps(int C, int m, const double *w, const double *mu, const double *var,
                         const double *y, double *slab, double *crps, hipStream_t s);
void launch_mixture_pair_rate(int iters, int blocks, double *out, hipStream_t s);
// ---- CRPS and mean after a monotone map (ngp_mixture_mapped_kernels.h) ----------------------
// The scan kernel leaves one record per date; the host plans the panels of a date from it
// (mixmap_plan) and relaunches only the dates that need a finer width.
// (constants, the per-date record, MixMapPlan and the planner: ngp_mixmap_plan.h — plain C++, so
// that the host tests can drive the planner on its own)
void launch_mixmap_scan(int C, int m, const ngp_inv_transform &inv, int scale, double shift,
                        const double *w, const double *mu, const double *invsd, const double *y,
                        double *rec, hipStream_t s);
void launch_mixmap_panels(int C, int nwork, int maxp, const ngp_inv_transform &inv, int scale,
                          double shift, const MixMapPlan *plans, const double *w, const double *mu,
                          const double *invsd, double *slab, double *res, hipStream_t s);
// ---- functionals of whole sample paths (ngp_path_kernels.h) ---------------------------------
constexpr int PATH_LCHUNK = 2048;      // doubles of L staged in LDS at a time (whole rows)
constexpr int PATH_SLICE = 4096;       // values per workgroup in the reduce and select passes
constexpr int PATH_MAX_TARGETS = 64, PATH_MAX_LEVELS = 64;
// paths per workgroup of path_values_kernel: L's chunk plus the state [m][PW] stay within 80 KiB
// (two workgroups per CU) up to m = 64; beyond, one wave's worth of paths (114,688 B at m = 192)
inline int path_pw(int m) { return m <= 32 ? 256 : m <= 64 ? 128 : 64; }
inline size_t path_lds_bytes(int m, int PW) { return 8 * ((size_t)PATH_LCHUNK + (size_t)m * PW); }
constexpr int PATH_LDS_MAX = 8 * (PATH_LCHUNK + NGP_MAX_AUX * 64);
static_assert(PATH_LCHUNK >= NGP_MAX_AUX, "a chunk holds at least one row of L");
static_assert(PATH_LDS_MAX <= 160 * 1024, "the state of 64 paths at NGP_MAX_AUX dates fits the LDS");
inline int64_t path_slices(int64_t N) { return (N + PATH_SLICE - 1) / PATH_SLICE; }
// an upper bound of sum_b ceil(cnt_b / PW) over B buckets that hold N paths
inline int64_t path_values_grid(int64_t N, int64_t B, int PW) { return N / PW + std::min(N, B) + 1; }
struct PathGeom {
    int32_t P, S, m, draws;
    int32_t B;         // buckets: P (shared components) or S P (independent mixtures)
    int32_t indep, PW;
    int32_t T, Tr, R;  // targets, the real-valued ones among them, distinct ranks asked for
    int64_t N;         // S draws
};
struct PathBufs {
    const double *w, *mu;          // as ngp_mixture_sample(_indep) takes them
    double *chol;                  // sigma in, L out
    const uint64_t *seeds;         // [S] or null
    int32_t *info;                 // [B]
    int32_t *bkt, *order;          // [N]
    uint32_t *rank, *cnt, *off, *wgoff;   // [N], [B], [B + 1], [B + 1]
    const ngp_path_target *targets;       // [T]
    const int32_t *real;           // [Tr] the real-valued targets
    const int64_t *ranks;          // [R] ascending, distinct, 1-based
    double *values, *partial, *mean;      // [T][N], [T][path_slices(N)], [T]
    unsigned long long *count, *hist;     // [T], [T][m]
    unsigned long long *prefix, *gpre;    // [Tr][R]
    long long *krem;               // [Tr][R]
    int32_t *grp, *ng;             // [Tr][R], [Tr]
    uint32_t *ghist;               // [Tr][R][256]
    double *q;                     // [Tr][R]
};
hipError_t launch_path_targets(const PathGeom &g, const PathBufs &p, const ngp_inv_transform &inv,
                               uint64_t seed, hipStream_t s);
// ---- energy score and sample CRPS of an ensemble of paths (ngp_score_kernels.h) ---------------
// The pair term is cut into SCORE_TILE x SCORE_TILE tiles of the upper triangle of (path, path),
// one partial per (tile, window) in slab [score_tile_pairs(N)][W]; term_obs leaves one partial per
// (slice of SCORE_THREADS paths, window).  Both slabs are then folded SCORE_REDUCE rows at a time,
// in row order, until one row is left.
constexpr int SCORE_THREADS = 256;
constexpr int SCORE_TILE = 128;        // paths per tile side: a thread owns 8 x 8 pairs
constexpr int SCORE_DCHUNK = 16;       // dates of both tiles staged in LDS at a time (32 KiB)
constexpr int SCORE_FOLD = 2048;       // dates after which a squared distance moves to a second accumulator
constexpr int SCORE_REDUCE = 2048;     // rows of a slab one workgroup folds
constexpr int SCORE_GRID_X = 1 << 23;    // workgroups per row of the pair kernel's grid: 2^31 threads, below the launch limit of 2^32
constexpr int SCORE_MAX_PATHS = 1 << 20, SCORE_MAX_WINDOWS = 4096, SCORE_MAX_DATES = 65535;
static_assert(SCORE_FOLD % SCORE_DCHUNK == 0, "a fold falls on a chunk boundary");
inline int64_t score_tiles(int64_t N) { return (N + SCORE_TILE - 1) / SCORE_TILE; }
inline int64_t score_tile_pairs(int64_t N) { const int64_t nt = score_tiles(N); return nt * (nt + 1) / 2; }
inline int64_t score_slices(int64_t N) { return (N + SCORE_THREADS - 1) / SCORE_THREADS; }
inline int64_t score_folded(int64_t rows) { return (rows + SCORE_REDUCE - 1) / SCORE_REDUCE; }
struct ScoreBufs {
    const double *x, *y;           // [N][m] paths (path-major), [m] observations, original scale
    double *u, *v;                 // [m][N] s(paths), [m] s(y)
    int32_t *flag;                 // [m] nonzero: a value of that date is not finite on the score scale (zeroed by the launcher)
    const int32_t *win;            // [W][2]
    double *pair[2], *obs[2];      // slabs: [score_tile_pairs(N)][W] / [score_folded(..)][W]; [score_slices(N)][W] / [score_folded(..)][W]
};
// inv: the inverse transformation applied to x first, or null.  obs_sum / pair_sum: where the [W]
// totals (before the division by N and D) are left, inside the slabs.
hipError_t launch_scores(int N, int m, int W, bool long_windows, const ngp_inv_transform *inv,
                         int scale, double shift, const ScoreBufs &b, const double **obs_sum,
                         const double **pair_sum, hipStream_t s);
// ---- the leapfrog step of ngp_grad_job_hmc (ngp_hmc_kernels.h) -------------------------------
// INIT writes theta(z0) for evaluation 0; FIRST, MIDDLE and LAST follow evaluations 0, 1 .. L - 1
// and L of a trajectory of L leapfrogs.
enum { HMC_INIT = 0, HMC_FIRST = 1, HMC_MIDDLE = 2, HMC_LAST = 3 };
struct HmcDev {
    DevProgram *progs;             // [B] the leaf's programs: params[] / noise are written
    const double *grad, *logml;    // the leaf's d_grad [B][NGP_MAX_PARAMS + 1], d_logml [B]
    const int32_t *info;           // d_info [B]
    const int32_t *off;            // [B + 1] an item's first latent in the flat arrays below
    const uint8_t *slot;           // per latent: its device parameter slot (the noise: n_params)
    const uint8_t *kind, *frozen;  // per latent
    double *z, *pm, *theta;        // per latent, the caller's order
    double *trace;                 // null, or the row of z_trace this step fills
    double *U0, *K0, *U1, *K1, *lm1;   // [B]
    int32_t *info1;                // [B]
    double eps, mu[5], sigma[5];
    int32_t B, phase;
};
void launch_hmc_step(const HmcDev &a, hipStream_t s);
void launch_mfma_bench(double *out, int iters, int blocks, hipStream_t s);
void launch_mfma_bench_detail(unsigned long long *stamps, int iters, int blocks, hipStream_t s);
void launch_mfma_layout_probe(const double *A, const double *Bm, double *Dout, hipStream_t s);
void launch_stream_write(double *dst, int64_t n, hipStream_t s);
void launch_stream_copy(double *dst, const double *src, int64_t n, hipStream_t s);

}  // namespace ngp

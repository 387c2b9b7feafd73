// ngp_kernels.hip — hand-written gfx950 (CDNA4) kernels of the GP hot path.
//
// Data layout in HBM (per item = one particle's covariance kernel), row-major fp64:
//   factor storage  [(n0 + naux_pad) x n0]:
//       rows [0, n0)            K(t0,t0)+(noise+jitter)I, lower 64x64 blocks only; overwritten in
//                               place by its Cholesky factor L, one 64-wide block column per step
//       rows [n0, n0+naux)      "aux rows" X = [k(t_add,t0); k(t_new,t0); y0'] that ride along
//                               and become W = X L^-T (appended points, forecast points, data)
//   Everything downstream (log-marginal likelihoods for every scenario, predictive mean and
//   covariance) is Schur-complement algebra on the small Gram matrix G = W W'.
//
// Where the kernels are:
//   ngp_tree_kernels.h    everything that evaluates a kernel tree: the interpreters and their shared
//                         helpers, cov_kernel, tables_kernel, the four fill kernels, kapply_kernel
//   ngp_grad_kernels.h    grad_kinv*, grad_alpha, the three grad_contract* kernels, toep_*, grad_reduce
//   ngp_col_kernels.h     chol_diag_kernel and the column kernels; ngp_small_kernels.h: short series
//                         in one launch; ngp_mixture_kernels.h: mixture summaries;
//                         ngp_component_kernels.h: fill and epilogue of ngp_factor_components;
//                         ngp_long_kernels.h: ngp_factor_predict_long (the dates as a solve's panel);
//                         ngp_long_sample_kernels.h: ngp_factor_sample_long (paths from its sigma);
//                         ngp_long_sample_indep_kernels.h: ngp_factor_sample_long_indep (its pick and normals);
//                         ngp_long_component_kernels.h: ngp_factor_components_long (component rows in its panel);
//                         ngp_long_origin_kernels.h: ngp_factor_predict_origins (prefixes of its solved rows);
//                         ngp_path_kernels.h: functionals of whole sample paths
//   this file             aux_update / aux_back_* / refine_gram_* (resident factor, Gram refinement),
//                         diag_ahead, gram, epilogue, mixture sampling, the probe and stream kernels,
//                         and every launcher
//
// Kernels (roofline class):
//   tables_kernel / fill_lattice_kernel / fill_single_kernel / fill_chain_kernel
//                     table-driven covariance fill on lattice times
//   fill_kernel       direct RPN kernel-tree interpreter, one 64x64 tile per workgroup, 512-B row
//                     stores                                   (HBM-write + fp64 transcendental VALU)
//   chol_diag_kernel  C_jj -= L_j L_j' (MFMA), 64x64 Cholesky four pivots per barrier round on
//                     packed lower-triangular LDS tiles, full inverse M = L_jj^-1 in MFMA strip
//                     order                                                 (latency-bound)
//   chol_col_glds_kernel / chol_col_kernel   C_rj -= L_r L_j' (v_mfma_f64_4x4x4_4b_f64 composite,
//                     64x64 tile per wave, LDS-DMA staged operands on the long k-loops), then the
//                     64-wide solve L_rj = C_rj M' on the accumulators (fp64-MFMA-bound; dominant)
//   diag_ahead_kernel pre-accumulation of the next-but-one diagonal tile on a side stream
//   gram_kernel       G = W W'                                              (HBM-read-bound, small)
//   epilogue_kernel   dense Schur algebra per item + per-scenario solves     (latency-bound, tiny)
//   grad_*            K^-1 = W_I W_I' (MFMA), reverse-mode contraction with aa' - K^-1
//   aux_update_kernel right-looking sweep of the aux rows through a resident factor
//
// MFMA operand maps used throughout (v_mfma_f64_16x16x4_f64, guide cdna_hip_programming.md §3):
//   A: lane l holds A[m = l&15][k = l>>4]     B: lane l holds B[k = l>>4][n = l&15]
//   D: lane l, register r holds D[m = (l>>4) + 4 r][n = l&15]
// so a D-layout tile is directly the B operand of a following product that sums over its row
// index (register r <-> k-slot), which is what keeps the triangular solve in registers.
#include "ngp_internal.h"
#include "ngp_mfma.h"
#include "ngp_col_kernels.h"
#include "ngp_small_kernels.h"
#include "ngp_mixture_kernels.h"
#include "ngp_tree_kernels.h"
#include "ngp_component_kernels.h"
#include "ngp_long_kernels.h"
#include "ngp_long_component_kernels.h"
#include "ngp_long_origin_kernels.h"
#include "ngp_grad_kernels.h"
#include "ngp_hmc_kernels.h"

namespace ngp {

// order[slot] = the item with the slot-th largest number of fp64 tile products since the previous
// call (mixcnt[2 i + 1] counts them; prev keeps the snapshot), ties by index.  One workgroup.
__global__ __launch_bounds__(256) void mixed_order_kernel(const unsigned *mixcnt, unsigned *prev,
                                                          int32_t *order, int Bc) {
    extern __shared__ unsigned keys[];
    for (int i = threadIdx.x; i < Bc; i += 256) {
        const unsigned now = mixcnt[2 * i + 1];
        keys[i] = now - prev[i];
        prev[i] = now;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < Bc; i += 256) {
        const unsigned k = keys[i];
        int rank = 0;
        for (int o = 0; o < Bc; ++o) rank += (keys[o] > k) || (keys[o] == k && o < i);
        order[rank] = i;
    }
}

// diag-ahead: K_(j+2,j+2) -= L_(j+2),[0,kmax) L_(j+2),[0,kmax)' — one workgroup per item, next to
// the fat launch (pre-accumulates the next-but-one diagonal tile so chol_diag's own k-loop is
// <= 128).  NW waves split the k-range and add their partial tiles in wave order through LDS: with
// few items and a long history (64 particles at n = 8192) a single wave per item took 0.8 ms per
// launch and the main stream waited for it at every second block column.
template <int NW>
__global__ __launch_bounds__(64 * NW, 2) void diag_ahead_kernel(JobGeom g, ChunkPtrs p, int j) {
    __shared__ double part[NW > 1 ? 64 * 64 : 1];   // [register][lane]: conflict-free
    const int item = blockIdx.x, lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long ld = g.ld;
    double *Ld = p.L + (long)item * g.item_stride + (long)(j + 2) * NB * ld;
    const int r16 = lane & 15, q = lane >> 4;
    double acc4[4][4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc4[a][b][r] = 0.0;
    const double *pd = Ld + (long)r16 * ld + 2 * q;
    // k-range in NW pieces, each a multiple of 16 (gemm_rows' stage depth)
    const int kmax = j * NB, per = ((kmax / 16 + NW - 1) / NW) * 16;
    const int k0 = min(wave * per, kmax), k1 = min(k0 + per, kmax);
    // Self-product of the 64 rows: both 64-byte halves of a row's 128-byte line are requested
    // together, one 16-deep stage ahead.  (gemm_rows asks for the halves one MFMA stage apart, and
    // the PMC counters showed every line of these rows fetched from HBM twice: 1.85 x the
    // algorithmic bytes, profiles/r02/README.md.)  Same MFMA order as gemm_rows: bit-identical.
    if (k1 > k0) {
        Frag8<4> f[2][2];
        load_frag8(f[0][0], pd + k0, ld);
        load_frag8(f[0][1], pd + k0 + 8, ld);
        for (int kc = k0; kc < k1; kc += 32) {
            if (kc + 16 < k1) {
                load_frag8(f[1][0], pd + kc + 16, ld);
                load_frag8(f[1][1], pd + kc + 24, ld);
            }
            mfma_frag8(acc4, f[0][0], f[0][0]);
            mfma_frag8(acc4, f[0][1], f[0][1]);
            if (kc + 16 < k1) {
                if (kc + 32 < k1) {
                    load_frag8(f[0][0], pd + kc + 32, ld);
                    load_frag8(f[0][1], pd + kc + 40, ld);
                }
                mfma_frag8(acc4, f[1][0], f[1][0]);
                mfma_frag8(acc4, f[1][1], f[1][1]);
            }
        }
    }
    if constexpr (NW > 1) {
        for (int w = 1; w < NW; ++w) {          // wave w adds its tile; wave 0 collects last
            if (wave == w) {
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            double *e = &part[((a * 4 + b) * 4 + r) * 64 + lane];
                            *e = (w == 1) ? acc4[a][b][r] : *e + acc4[a][b][r];
                        }
            }
            __syncthreads();
        }
        if (wave != 0) return;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc4[a][b][r] += part[((a * 4 + b) * 4 + r) * 64 + lane];
    }
    subtract_in_place_perm(Ld, ld, (j + 2) * NB, acc4, lane);
}

// cached factor (ngp_factor_*): L and every M_j stay on the device; a query only needs its aux
// rows W = X L^-T.  Right-looking sweep over block columns, so each step is wide instead of a
// long k-loop on a single wave per aux tile:  W_j = C_j M_j' (chol_col_kernel, empty k-range),
// then this kernel:  C_c -= W_j L_(c,j)'  for every block column c > j, one wave per (aux tile, c).
__global__ __launch_bounds__(256, 2) void aux_update_kernel(JobGeom g, ChunkPtrs p, int j) {
    const int item = p.items ? p.items[blockIdx.y] : blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ntl = g.naux_pad / NB;
    const int idx = blockIdx.x * 4 + wave;
    if (idx >= ntl * (g.nb0 - 1 - j)) return;
    const int a = idx % ntl, c = j + 1 + idx / ntl;
    const long ld = g.ld;
    double *Lit = p.L + (long)item * g.item_stride;
    double *Wa = Lit + ((long)g.n0 + (long)a * NB) * ld;      // aux tile rows (B operand)
    const double *Lc = Lit + (long)c * NB * ld;               // rows of block c (A operand)
    const int r16 = lane & 15, q = lane >> 4;
    double acc4[4][4][4];
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc4[x][y][r] = 0.0;
    gemm_rows<4>(acc4, Lc + (long)r16 * ld + 2 * q, Wa + (long)r16 * ld + 2 * q, ld, j * NB,
                 (j + 1) * NB);
    subtract_in_place_perm(Wa, ld, c * NB, acc4, lane);
}

// ---------------------------------------------------------------------------------------
// Gram refinement of NGP_PREC_MIXED jobs.  X = the aux rows as filled ([k(t_aux, t0) ; y']), P = L L'
// the mixed-precision factor, K the exact fp64 covariance.  With A ~ X K^-1:
//     R = X - A K                      (kapply_kernel: K re-evaluated tile by tile, never stored)
//     G = A X' + R A'                  (refine_gram_*: second-order accurate in the error of A)
//     A += (R L^-T) L^-1               (forward sweep = the resident-factor kernels; backward sweep
//                                       = aux_back_kernel)
// A_0 = W L^-1 from the W = X L^-T the factorisation leaves in the aux rows.
// ---------------------------------------------------------------------------------------
// position of M[R][C] inside the strip-ordered block inverse chol_diag writes
__device__ __forceinline__ int mstrip_index(int R, int C) {
    return (((R >> 2) * 4 + (C >> 4)) << 6) + (R & 3) + 4 * ((C >> 2) & 3) + 16 * (C & 3);
}

// Backward sweep, block column c (c descending across launches), two launches per block column:
//   aux_back_solve_kernel   A_c = C_c L_cc^-1 = C_c M_c, in place in the aux rows and out to Aout
//                           ([Bc][naux_pad][n0]; accumulate: +=); one workgroup per (aux tile, item)
//   aux_back_update_kernel  C_b -= A_c L_(c,b) for every b < c; one wave per (aux tile, b), the same
//                           4x4x4 MFMA tile product as the forward sweep with the L tile read
//                           transposed (k runs down its rows)
__global__ __launch_bounds__(256) void aux_back_solve_kernel(JobGeom g, ChunkPtrs p,
                                                             const double *Mc, double *Aout,
                                                             int accumulate, int c) {
    __shared__ double Ms[NB][NB + 1];   // M = L_cc^-1, natural layout
    __shared__ double Cs[NB][NB + 1];   // the aux tile's block column c
    const int item = map_item(p, blockIdx.y), at = blockIdx.x, tid = threadIdx.x;
    const long ld = g.ld;
    double *Caux = p.L + (long)item * g.item_stride + ((long)g.n0 + (long)at * NB) * ld + c * NB;
    const double *M = Mc + (long)item * (NB * NB);
    const int rows = min(NB, g.naux - at * NB);
    for (int e = tid; e < NB * NB; e += 256) {
        const int i = e >> 6, jj = e & 63;
        Ms[i][jj] = (i >= jj) ? M[mstrip_index(i, jj)] : 0.0;
        Cs[i][jj] = (i < rows) ? Caux[(long)i * ld + jj] : 0.0;
    }
    __syncthreads();
    const int jc = tid & 63, w = tid >> 6;
    for (int a = w; a < rows; a += 4) {
        double sum = 0.0;
        for (int i = jc; i < NB; ++i) sum += Cs[a][i] * Ms[i][jc];
        Caux[(long)a * ld + jc] = sum;
        double *dst = Aout + ((long)item * g.naux_pad + at * NB + a) * ld + c * NB + jc;
        *dst = accumulate ? *dst + sum : sum;
    }
}

// 8 k-values of four 16-row fragments of a TRANSPOSED operand: element (m, k) lives at p[k * ld + m]
// (lane (r16, q): rows m = 16 u + r16, k = 2 q, 2 q + 1)
__device__ __forceinline__ void load_frag8_t(Frag8<4> &f, const double *p, long ld) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        f.v[u].x = p[16 * u];
        f.v[u].y = p[ld + 16 * u];
    }
}

// NIT: 16-row groups of the aux tile that hold real rows (1 for the usual d + m + 1 <= 16, else 4).
// The four waves of a workgroup take four different b and share A_c through LDS.
template <int NIT>
__global__ __launch_bounds__(256, 2) void aux_back_update_kernel(JobGeom g, ChunkPtrs p, int c) {
    constexpr int PITCH = NB + 2;
    __shared__ __attribute__((aligned(16))) double Acs[16 * NIT][PITCH];
    const int item = map_item(p, blockIdx.y);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ngrp = (c + 3) / 4;                    // workgroups per aux tile
    const int at = blockIdx.x / ngrp, b = (blockIdx.x % ngrp) * 4 + wave;
    const long ld = g.ld;
    double *Lit = p.L + (long)item * g.item_stride;
    double *Wa = Lit + ((long)g.n0 + (long)at * NB) * ld;          // aux tile rows
    for (int e = threadIdx.x; e < 16 * NIT * NB; e += 256) {
        const int r = e >> 6, k = e & 63;
        Acs[r][k] = Wa[(long)r * ld + c * NB + k];                 // A_c (aux_back_solve_kernel)
    }
    __syncthreads();
    if (b >= c) return;
    const double *Lcb = Lit + (long)c * NB * ld + (long)b * NB;    // L tile (c, b), read transposed
    const int r16 = lane & 15, q = lane >> 4;
    double acc4[4][NIT][4];
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < NIT; ++y)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc4[x][y][r] = 0.0;
    // S'[jj][a] = sum_k L[64 c + k][64 b + jj] A_c[a][k]
    const double *pa = Lcb + (long)(2 * q) * ld + r16;
    Frag8<4> a[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) load_frag8_t(a[s], pa + (long)(8 * s) * ld, ld);   // whole tile in flight
#pragma unroll
    for (int s = 0; s < 8; ++s) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const f64x2 bv = *reinterpret_cast<const f64x2 *>(&Acs[16 * it + r16][8 * s + 2 * q]);
            const Rot4 bx = rot4(bv.x);
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) mfma16_as_4(acc4[jt][it], a[s].v[jt].x, bx);
            const Rot4 by = rot4(bv.y);
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) mfma16_as_4(acc4[jt][it], a[s].v[jt].y, by);
        }
    }
    // Wa[a][64 b + jj] -= S'[jj][a]
    const int jj0 = 4 * (r16 >> 2) + q;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int it = 0; it < NIT; ++it)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double *e = Wa + (long)(16 * it + ((r16 + 4 * r) & 15)) * ld + b * NB + 16 * jt + jj0;
                *e -= acc4[jt][it][r];
            }
}

// S[a][b] = A_a . X_b + R_a . A_b and T[a][b] = R_a . A_b for all naux^2 pairs, one wave per pair
__global__ __launch_bounds__(256) void refine_gram_pairs_kernel(JobGeom g, const double *A,
                                                                const double *X, const double *R,
                                                                double *S, double *T, double *U,
                                                                const int32_t *items) {
    const int item = items ? items[blockIdx.y] : blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pr = blockIdx.x * 4 + wave;
    if (pr >= g.naux * g.naux) return;
    const int a = pr / g.naux, b = pr % g.naux;
    const long base = (long)item * g.naux_pad * g.ld;
    const double *Aa = A + base + (long)a * g.ld, *Ab = A + base + (long)b * g.ld;
    const double *Xb = X + base + (long)b * g.ld, *Ra = R + base + (long)a * g.ld;
    double s0 = 0.0, t0 = 0.0, rr = 0.0, xx = 0.0;
    for (int k = lane; k < g.n0; k += 64) {
        s0 += Aa[k] * Xb[k];
        t0 += Ra[k] * Ab[k];
        if (a == b) {   // wave-uniform: |R_a|^2 and |X_a|^2 for the contraction estimate
            rr += Ra[k] * Ra[k];
            xx += Xb[k] * Xb[k];
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s0 += __shfl_down(s0, off, 64);
        t0 += __shfl_down(t0, off, 64);
        rr += __shfl_down(rr, off, 64);
        xx += __shfl_down(xx, off, 64);
    }
    if (lane == 0) {
        S[(long)item * g.naux * g.naux + pr] = s0 + t0;
        T[(long)item * g.naux * g.naux + pr] = t0;
        if (a == b) U[(long)item * g.naux + a] = xx > 0.0 ? rr / xx : 0.0;
    }
}

// G = (S + S') / 2;  delta[2 item] = max |T + T'| / 2 relative to sqrt(G_aa G_bb), the size of the
// correction this step applied;  delta[2 item + 1] = max_a |R_a| / |X_a|, how far (L L')^-1 K is
// from the identity along the rows of X (the factor by which the next correction is smaller)
__global__ __launch_bounds__(256) void refine_gram_final_kernel(JobGeom g, const double *S,
                                                                const double *T, const double *U,
                                                                double *G, double *delta,
                                                                const int32_t *items) {
    __shared__ double red[256];
    const int item = items ? items[blockIdx.x] : blockIdx.x;
    const int tid = threadIdx.x, na = g.naux;
    const double *Si = S + (long)item * na * na, *Ti = T + (long)item * na * na;
    double *Gi = G + (long)item * na * na;
    double dm = 0.0;
    for (int e = tid; e < na * na; e += 256) {
        const int a = e / na, b = e % na;
        Gi[e] = 0.5 * (Si[a * na + b] + Si[b * na + a]);
        const double gaa = Si[a * na + a], gbb = Si[b * na + b];
        const double den = sqrt(fabs(gaa * gbb));
        const double tv = 0.5 * fabs(Ti[a * na + b] + Ti[b * na + a]);
        // fmax drops NaN: a non-finite correction must come out as NaN (the item is then
        // never marked refined), so it is carried explicitly
        if (!(tv == tv) || !(den == den)) dm = NAN;
        else if (dm == dm) {
            if (den > 0.0) dm = fmax(dm, tv / den);
            else if (tv > 0.0) dm = INFINITY;
        }
    }
    red[tid] = dm;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) {
            const double a = red[tid], b = red[tid + off];
            red[tid] = (a == a && b == b) ? fmax(a, b) : NAN;
        }
        __syncthreads();
    }
    if (tid == 0) {
        delta[2 * item] = red[0];
        double rho2 = 0.0;
        for (int a = 0; a < na; ++a) {
            const double u = U[(long)item * na + a];
            rho2 = (u == u && rho2 == rho2) ? fmax(rho2, u) : NAN;
        }
        delta[2 * item + 1] = sqrt(rho2);
    }
}

// ---------------------------------------------------------------------------------------
// gram: G = W W' over the aux rows (lower triangle computed, mirrored on store)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gram_kernel(JobGeom g, const double *L, double *G) {
    const int item = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double *W = L + (long)item * g.item_stride + (long)g.n0 * g.ld;
    double *Go = G + (long)item * g.naux * g.naux;
    const int npairs = g.naux * (g.naux + 1) / 2;
    if (g.n0 <= 512) {
        // short rows: one pair per thread, a serial dot product over at most 512 elements that sit
        // in L1 (the wave-per-pair form below spends its time on index arithmetic and shuffles: 46 us
        // for 276 pairs at n0 = 128)
        for (int e = threadIdx.x; e < g.naux * g.naux; e += 256) {
            const int a = e / g.naux, b = e % g.naux;
            if (b > a) continue;
            const double *wa = W + (long)a * g.ld, *wb = W + (long)b * g.ld;
            double s0 = 0.0, s1 = 0.0;
            for (int k = 0; k < g.n0; k += 2) {
                s0 += wa[k] * wb[k];
                s1 += wa[k + 1] * wb[k + 1];
            }
            const double sv = s0 + s1;
            Go[a * g.naux + b] = sv;
            Go[b * g.naux + a] = sv;
        }
        return;
    }
    for (int pr = wave; pr < npairs; pr += 4) {
        int a, b;
        tri_decode(pr, a, b);
        const double *wa = W + (long)a * g.ld, *wb = W + (long)b * g.ld;
        double s = 0.0;
        for (int k = lane; k < g.n0; k += 64) s += wa[k] * wb[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if (lane == 0) {
            Go[a * g.naux + b] = s;
            Go[b * g.naux + a] = s;
        }
    }
}

// ---------------------------------------------------------------------------------------
// epilogue: Schur-complement algebra on G (one single-wave workgroup per item)
//   A = appended rows (da), T = forecast rows (m), Y = data row
//   S_AA = K_AA + nz I - G_AA = L_A L_A'        V_A = (K_TA - G_TA) L_A^-T
//   Sigma = K_TT - G_TT - V_A V_A' (+ nz I)     per scenario: z_A = L_A^-1 (y_A - G_AY)
//   logml_full = -1/2 (G_YY + |z_A|^2) - (logdet0 + sum log diag L_A) - (n+d)/2 log 2pi
//   mu = G_TY + V_A z_A ;  logml_base = same with the first `tail` appended rows only
// ---------------------------------------------------------------------------------------
// The working set (L_A, V_A, log diag) lives in dynamic LDS when it fits (lds_work != 0; the usual
// case: a ragged tail of < 64 points plus a few appended ones) — the pivot loop of the da x da
// factorisation is a chain of dependent accesses, 114 us from global memory against ~20 from LDS
// at da = 22 — and in the per-item global work buffer otherwise.
__global__ __launch_bounds__(64) void epilogue_kernel(JobGeom g, EpiPtrs p, DevSpec sp, int lds_work) {
    __shared__ DevProgram P;
    __shared__ int bad;
    extern __shared__ double epi_dyn[];
    const int item = blockIdx.x, tid = threadIdx.x;
    load_program(&P, p.progs + item);
    if (tid == 0) bad = 0;
    __syncthreads();
    const int da = g.da, m = g.m, na = g.naux, Y = da + m;
    const double nz = P.noise + sp.jitter;
    const double *G = p.G + (long)item * na * na;
    double *work = lds_work ? epi_dyn : p.work + (long)item * p.work_stride;
    // k(aux point u, aux point v): table lookups when the item's lattice tables are at hand
    const double *tab = p.tab ? p.tab + (long)item * g.maxstat * g.R : nullptr;
    const double *sig = p.sig ? p.sig + (long)item * g.maxcp * g.npts : nullptr;
    auto kaux = [&](int u, int v) -> double {   // u, v index taux: appended points then forecast points
        if (tab)
            return keval_reduced(P, tab, sig, g.R, g.npts, p.taux[u], p.taux[v],
                                 abs(p.qpts[g.n0 + u] - p.qpts[g.n0 + v]), g.n0 + u, g.n0 + v);
        return keval(P, sp, p.taux[u], p.taux[v]);
    };
    double *LA = work;                  // [da x da]
    double *VA = LA + (long)da * da;    // [m x da]
    double *ldA = VA + (long)m * da;    // [da] log diag L_A

    for (int e = tid; e < da * da; e += 64) {
        const int a = e / da, b = e % da;
        double v = 0.0;
        if (b <= a) {
            v = kaux(a, b) - (g.n0 ? G[a * na + b] : 0.0);
            if (a == b) v += nz;
        }
        LA[e] = v;
    }
    __syncthreads();
    for (int k = 0; k < da; ++k) {  // in-place right-looking Cholesky of S_AA (one wave: row per thread)
        const double akk = LA[k * da + k];
        const double dk = sqrt(akk);
        __syncthreads();
        if (tid == 0) {
            if (!(akk > 0.0) && bad == 0) bad = k + 1;
            LA[k * da + k] = dk;
        }
        for (int i = k + 1 + tid; i < da; i += 64) LA[i * da + k] /= dk;
        __syncthreads();
        for (int i = k + 1 + tid; i < da; i += 64) {
            const double lik = LA[i * da + k];
            for (int jj = k + 1; jj <= i; ++jj) LA[i * da + jj] -= lik * LA[jj * da + k];
        }
        __syncthreads();
    }
    for (int a = tid; a < da; a += 64) ldA[a] = log(LA[a * da + a]);
    __syncthreads();
    // V_A: one forecast row per thread, forward substitution along the appended points
    for (int i = tid; i < m; i += 64) {
        for (int a = 0; a < da; ++a) {
            double s = kaux(da + i, a) - (g.n0 ? G[(da + i) * na + a] : 0.0);
            for (int pp = 0; pp < a; ++pp) s -= VA[i * da + pp] * LA[a * da + pp];
            VA[i * da + a] = s / LA[a * da + a];
        }
    }
    __syncthreads();
    if (p.sigma) {
        double *Sg = p.sigma + (long)item * m * m;
        for (int e = tid; e < m * m; e += 64) {
            const int i = e / m, jj = e % m;
            if (jj > i) continue;
            double s = kaux(da + i, da + jj) - (g.n0 ? G[(da + i) * na + da + jj] : 0.0);
            for (int a = 0; a < da; ++a) s -= VA[i * da + a] * VA[jj * da + a];
            if (i == jj && g.noise_on_new) s += nz;
            Sg[i * m + jj] = s;
            Sg[jj * m + i] = s;
        }
    }
    const double q0 = g.n0 ? G[Y * na + Y] : 0.0;
    const double ld0 = p.logdet[item];
    const double LOG2PI = 1.8378770664093454836;
    const double *ya_base = p.ya + (g.y_shared ? 0 : (long)item * g.D * da);
    if (g.D <= 8) {
        // few scenarios (a logml / predict call): the wave solves them one after the other, every
        // row's dot product spread over the lanes, instead of one long serial loop on one lane
        for (int s = 0; s < g.D; ++s) {
            const double *ya = ya_base + (long)s * da;
            double *z = p.zbuf + ((long)item * g.D + s) * da;
            double quad = 0.0, quad_tail = 0.0, ldsum = 0.0, ld_tail = 0.0;
            for (int a = 0; a < da; ++a) {
                double part = 0.0;
                for (int pp = tid; pp < a; pp += 64) part += LA[a * da + pp] * z[pp];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
                const double e = (ya[a] - (g.n0 ? G[a * na + Y] : 0.0) - part) / LA[a * da + a];
                if (tid == 0) z[a] = e;
                __syncthreads();
                quad += e * e;
                ldsum += ldA[a];
                if (a < g.tail) { quad_tail += e * e; ld_tail += ldA[a]; }
            }
            const int nfull = g.n0 + da;
            if (tid == 0) {
                p.logml_full[(long)item * g.D + s] =
                    -0.5 * (q0 + quad) - (ld0 + ldsum) - 0.5 * nfull * LOG2PI;
                if (s == 0)
                    p.logml_base[item] =
                        -0.5 * (q0 + quad_tail) - (ld0 + ld_tail) - 0.5 * (g.n0 + g.tail) * LOG2PI;
            }
            if (p.mu) {
                double *mu = p.mu + ((long)item * g.D + s) * m;
                for (int i = tid; i < m; i += 64) {
                    double v = g.n0 ? G[(da + i) * na + Y] : 0.0;
                    for (int a = 0; a < da; ++a) v += VA[i * da + a] * z[a];
                    mu[i] = v;
                }
            }
        }
    } else {
    for (int s = tid; s < g.D; s += 64) {
        const double *ya = ya_base + (long)s * da;
        double *z = p.zbuf + ((long)item * g.D + s) * da;
        double quad = 0.0, quad_tail = 0.0, ldsum = 0.0, ld_tail = 0.0;
        for (int a = 0; a < da; ++a) {
            double e = ya[a] - (g.n0 ? G[a * na + Y] : 0.0);
            for (int pp = 0; pp < a; ++pp) e -= LA[a * da + pp] * z[pp];
            e /= LA[a * da + a];
            z[a] = e;
            quad += e * e;
            ldsum += ldA[a];
            if (a < g.tail) { quad_tail += e * e; ld_tail += ldA[a]; }
        }
        const int nfull = g.n0 + da;
        p.logml_full[(long)item * g.D + s] = -0.5 * (q0 + quad) - (ld0 + ldsum) - 0.5 * nfull * LOG2PI;
        if (s == 0)
            p.logml_base[item] =
                -0.5 * (q0 + quad_tail) - (ld0 + ld_tail) - 0.5 * (g.n0 + g.tail) * LOG2PI;
        if (p.mu) {
            double *mu = p.mu + ((long)item * g.D + s) * m;
            for (int i = 0; i < m; ++i) {
                double v = g.n0 ? G[(da + i) * na + Y] : 0.0;
                for (int a = 0; a < da; ++a) v += VA[i * da + a] * z[a];
                mu[i] = v;
            }
        }
    }
    }
    // (info < 0 is NGP_INFO_NOT_REFINED of a mixed-precision job, set before the epilogue ran: a pivot
    // failure in the tail or the appended points is the stronger statement and replaces it)
    if (tid == 0 && bad && p.info[item] <= 0) p.info[item] = g.n0 + bad;
}

// ---------------------------------------------------------------------------------------
// mixture sampling (ngp_mixture_sample)
// ---------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11):
// counter-based, so draw d of scenario s is a pure function of (seed, s, d) — no state to
// carry, any launch geometry gives the same stream.
struct Philox4 { unsigned x, y, z, w; };
__host__ __device__ inline Philox4 philox4x32_10(Philox4 c, unsigned k0, unsigned k1) {
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c.x, p1 = 0xCD9E8D57ull * c.z;
        const Philox4 n{(unsigned)(p1 >> 32) ^ c.y ^ k0, (unsigned)p1,
                        (unsigned)(p0 >> 32) ^ c.w ^ k1, (unsigned)p0};
        c = n;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}
// 53-bit uniform in (0, 1) from two 32-bit words
__host__ __device__ inline double u01(unsigned hi, unsigned lo) {
    const unsigned long long v = (((unsigned long long)hi << 32) | lo) >> 11;
    return ((double)v + 0.5) * (1.0 / 9007199254740992.0);
}

// in-place lower Cholesky of one m x m matrix per workgroup (row-major, upper part zeroed)
__global__ __launch_bounds__(256) void small_chol_kernel(double *A, int m, int32_t *info) {
    double *a = A + (long)blockIdx.x * m * m;
    __shared__ double piv;
    __shared__ int bad;
    const int tid = threadIdx.x;
    if (tid == 0) bad = 0;
    __syncthreads();
    for (int k = 0; k < m; ++k) {
        if (tid == 0) {
            const double akk = a[(long)k * m + k];
            if (!(akk > 0.0) && bad == 0) bad = k + 1;
            piv = sqrt(akk);
            a[(long)k * m + k] = piv;
        }
        __syncthreads();
        const double d = piv;
        for (int i = k + 1 + tid; i < m; i += 256) a[(long)i * m + k] /= d;
        __syncthreads();
        // trailing update, lower part: element (i, j), k < j <= i
        const int nt = m - k - 1;
        for (int e = tid; e < nt * nt; e += 256) {
            const int i = k + 1 + e / nt, j = k + 1 + e % nt;
            if (j <= i) a[(long)i * m + j] -= a[(long)i * m + k] * a[(long)j * m + k];
        }
        __syncthreads();
    }
    for (int e = tid; e < m * m; e += 256)
        if (e % m > e / m) a[e] = 0.0;
    if (tid == 0 && info) info[blockIdx.x] = bad;
}

// one thread per (scenario, draw).  seeds == nullptr: the S mixtures share their P components
// (mu [P][S][m], chol [P][m][m]) and one key, the scenario index is part of the counter.
// seeds != nullptr: S independent mixtures (mu [S][P][m], chol [S][P][m][m]); mixture s is keyed
// by seeds[s] with scenario counter 0, i.e. it draws exactly what a call with S = 1 and
// seed = seeds[s] draws.
__global__ __launch_bounds__(256) void mixture_sample_kernel(int P, int S, int m, const double *w,
                                                             const double *mu, const double *chol,
                                                             int draws, unsigned k0, unsigned k1,
                                                             const unsigned long long *seeds,
                                                             double *out, int32_t *comp) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)S * draws) return;
    const int s = (int)(idx / draws), d = (int)(idx % draws);
    unsigned cs = (unsigned)s;
    if (seeds) {
        k0 = (unsigned)seeds[s];
        k1 = (unsigned)(seeds[s] >> 32);
        cs = 0u;
    }
    // block 0: component pick by inverse CDF over the P weights of scenario s
    const Philox4 r0 = philox4x32_10(Philox4{(unsigned)d, cs, 0u, 0u}, k0, k1);
    const double u = u01(r0.x, r0.y);
    const double *ws = w + (long)s * P;
    int k = P - 1;
    double acc = 0.0;
    for (int i = 0; i < P; ++i) {
        acc += ws[i];
        if (u < acc) { k = i; break; }
    }
    if (comp) comp[idx] = k;
    // blocks 1..: four words -> one Box-Muller pair -> two normals
    const double *L = chol + ((seeds ? (long)s * P : 0l) + k) * m * m;
    const double *mk = mu + (seeds ? ((long)s * P + k) : ((long)k * S + s)) * m;
    double *o = out + idx * m;
    for (int i = 0; i < m; ++i) o[i] = mk[i];
    for (int j0 = 0; j0 < m; j0 += 2) {
        const Philox4 r = philox4x32_10(Philox4{(unsigned)d, cs, (unsigned)(1 + j0 / 2), 0u},
                                        k0, k1);
        const double u1 = u01(r.x, r.y), u2 = u01(r.z, r.w);
        const double rad = sqrt(-2.0 * log(u1)), ang = 2.0 * M_PI * u2;
        const double z0 = rad * cos(ang), z1 = rad * sin(ang);
        for (int i = j0; i < m; ++i) o[i] += L[(long)i * m + j0] * z0;          // column j0 of L
        if (j0 + 1 < m)
            for (int i = j0 + 1; i < m; ++i) o[i] += L[(long)i * m + j0 + 1] * z1;
    }
}

void launch_mixture_sample(int P, int S, int m, const double *w, const double *mu, double *chol,
                           int draws, uint64_t seed, const uint64_t *seeds, double *out,
                           int32_t *comp, int32_t *info, hipStream_t s) {
    const long mats = seeds ? (long)S * P : (long)P;
    hipLaunchKernelGGL(small_chol_kernel, dim3((unsigned)mats), dim3(256), 0, s, chol, m, info);
    const long n = (long)S * draws;
    hipLaunchKernelGGL(mixture_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P,
                       S, m, w, mu, (const double *)chol, draws, (unsigned)seed,
                       (unsigned)(seed >> 32), (const unsigned long long *)seeds, out, comp);
}

}  // namespace ngp
#include "ngp_path_kernels.h"   // uses philox4x32_10, u01 and small_chol_kernel above
#include "ngp_long_sample_kernels.h"   // uses philox4x32_10 and u01 above, chol_diag_kernel and the column kernels' tile code
#include "ngp_long_sample_indep_kernels.h"   // pick and normals of independent mixtures, behind the shared form's kernels
#include "ngp_mixture_mapped_kernels.h"   // uses path_inv and the block reductions of ngp_mixture_kernels.h
#include "ngp_score_kernels.h"   // uses path_inv and mix_block_sum
namespace ngp {

// ---------------------------------------------------------------------------------------
// microbenchmarks / self tests
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mfma_bench_kernel(double *out, int iters) {
    f64x4 c0 = {0, 0, 0, 0}, c1 = c0, c2 = c0, c3 = c0;
    const double a = 1.0 + 1e-9 * threadIdx.x, b = 1.0 - 1e-9 * threadIdx.x;
    for (int i = 0; i < iters; i += 4) {
        c0 = mfma64(a, b, c0);
        c1 = mfma64(a, b, c1);
        c2 = mfma64(a, b, c2);
        c3 = mfma64(a, b, c3);
    }
    const f64x4 r = c0 + c1 + c2 + c3;
    if (r[0] + r[1] + r[2] + r[3] == -1.0) out[blockIdx.x * 256 + threadIdx.x] = r[0];
}

// per-wave shader-clock cycles (s_memtime) and 100 MHz wall ticks (s_memrealtime) around the loop
__global__ __launch_bounds__(256) void mfma_bench_detail_kernel(unsigned long long *stamps,
                                                                int iters) {
    f64x4 c0 = {0, 0, 0, 0}, c1 = c0, c2 = c0, c3 = c0;
    const double a = 1.0 + 1e-9 * threadIdx.x, b = 1.0 - 1e-9 * threadIdx.x;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
    for (int i = 0; i < iters; i += 4) {
        c0 = mfma64(a, b, c0);
        c1 = mfma64(a, b, c1);
        c2 = mfma64(a, b, c2);
        c3 = mfma64(a, b, c3);
    }
    const f64x4 r = c0 + c1 + c2 + c3;
    asm volatile("" ::"v"(r[0]), "v"(r[1]), "v"(r[2]), "v"(r[3]));
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
    if ((threadIdx.x & 63) == 0) {
        const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
        stamps[2 * w] = t1 - t0;
        stamps[2 * w + 1] = r1 - r0;
    }
}

__global__ void mfma_layout_probe_kernel(const double *A, const double *Bm, double *Dout) {
    const int l = threadIdx.x;
    const double a = A[(l & 15) * 4 + (l >> 4)];    // A[m][k], 16x4 row-major
    const double b = Bm[(l >> 4) * 16 + (l & 15)];  // B[k][n], 4x16 row-major
    const f64x4 d = mfma64(a, b, (f64x4){0, 0, 0, 0});
#pragma unroll
    for (int r = 0; r < 4; ++r) Dout[((l >> 4) + 4 * r) * 16 + (l & 15)] = d[r];
}

__global__ void mfma4_composite_probe_kernel(const double *A, const double *Bm, double *Dout) {
    const int l = threadIdx.x;
    const double a = A[(l & 15) * 4 + (l >> 4)];
    const double b = Bm[(l >> 4) * 16 + (l & 15)];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    mfma16_as_4(acc, a, rot4(b));
    const f64x4 d = to_d16(acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) Dout[((l >> 4) + 4 * r) * 16 + (l & 15)] = d[r];
}

// D[32x32] = A[32x2] B[2x32] through one v_mfma_f32_32x32x2_f32 with the operand / result maps
// the mixed-precision k-loop assumes
__global__ void mfma_f32_probe_kernel(const float *A, const float *Bm, float *Dout) {
    const int l = threadIdx.x;
    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A[(l & 31) * 2 + (l >> 5)], Bm[(l >> 5) * 32 + (l & 31)],
                                               acc, 0, 0, 0);
#pragma unroll
    for (int v = 0; v < 16; ++v)
        Dout[((v & 3) + 8 * (v >> 2) + 4 * (l >> 5)) * 32 + (l & 31)] = acc[v];
}

__global__ __launch_bounds__(256) void stream_write_kernel(f64x2 *dst, long n2) {
    const f64x2 v = {1.0, 2.0};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n2; i += (long)gridDim.x * 256)
        dst[i] = v;
}
__global__ __launch_bounds__(256) void stream_copy_kernel(f64x2 *dst, const f64x2 *src, long n2) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n2; i += (long)gridDim.x * 256)
        dst[i] = src[i];
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
void launch_tables(const JobGeom &g, const ChunkPtrs &p, int Bc, const DevSpec &sp, hipStream_t s) {
    if (g.n0 == 0 || !g.lattice) return;
    JobGeom gt = g;
    // short gradient jobs fill on the full program (launch_fill): no subtree tables behind the leaves'
    if (p.dtab && small_job(g, Bc)) gt.tab_sub = 0;
    hipLaunchKernelGGL(tables_kernel, dim3(Bc), dim3(256), 0, s, gt, p, sp);
}

void launch_fill(const JobGeom &g, const ChunkPtrs &p, int Bc, const DevSpec &sp, hipStream_t s,
                 bool aux_only) {
    if (g.n0 == 0) return;
    const int ntri = g.nb0 * (g.nb0 + 1) / 2;
    // Gradient jobs (aux rows [I ; y']): the identity block is NOT written — the column kernels
    // synthesise a tile of it the first time they meet it (chol_col*<.., IDENT>).  What is written:
    // the tile row that carries y' and the zero blocks (a, a - 1) just left of the block diagonal,
    // which the k-loops of a tile pair and of K^-1 = W W' read as part of their shared k-range.
    const int ntiles = ntri + (g.aux_identity ? g.nb0 + (g.nb0 - 1) : (g.naux_pad / NB) * g.nb0);
    const int off = aux_only ? ntri : 0;
    const dim3 blk(256);
    // other / chain / single-table items of a chunk, each on its own kernel, over tiles [0, nt)
    auto by_shape = [&](int nt, int nt_single, int split) {
        // gradient jobs: the value kernels read the subtree tables behind the per-leaf ones
        ChunkPtrs lists = p;
        if (p.dtab) {
            lists.tab = p.tab + (size_t)g.tab_sub * g.R;
            lists.dtab = nullptr;
        }
        if (p.n_fill_other > 0)
            hipLaunchKernelGGL(fill_lattice_kernel<false>, dim3(nt * split, p.n_fill_other), blk, 0, s, g,
                               lists, ntri, 0, split, sp);
        if (p.n_fill_chain > 0) {
            const int tpw = tiles_per_wg((long)nt * p.n_fill_chain);
            hipLaunchKernelGGL(fill_chain_kernel, dim3((nt + tpw - 1) / tpw, p.n_fill_chain), blk, 0, s, g,
                               lists, ntri, sp, nt, tpw);
        }
        if (p.n_fill_single > 0)
            hipLaunchKernelGGL(fill_single_kernel, dim3(nt_single, p.n_fill_single), blk, 0, s, g, lists,
                               ntri, sp);
    };
    // tiles [first, first + nt) of every item on the general kernel (FULL: the gradient job's program)
    auto general = [&](auto kernel, int first, int nt) {
        ChunkPtrs whole = p;   // one kernel for every item of the chunk
        whole.fill_other = nullptr;
        const int split = launch_split((long)nt * Bc);
        hipLaunchKernelGGL(kernel, dim3(nt * split, Bc), blk, 0, s, g, whole, ntri, first, split, sp);
    };
    switch (fill_route(g, p.dtab != nullptr, p.fill_other != nullptr, Bc, aux_only)) {
    case FILL_DIRECT:
        hipLaunchKernelGGL(fill_kernel, dim3(ntiles - off, Bc), blk, 0, s, g, p, ntri, off, sp);
        break;
    case FILL_GRAD_SMALL:   // main tiles only (y' comes from the observations)
        general(fill_lattice_kernel<true>, 0, ntri);
        break;
    case FILL_GRAD_LISTS:
        // The main tiles through the kernels of the value jobs — one lookup for a stationary tree,
        // chain programs decoded once per thread for sixteen elements, the rest on the reduced
        // program; the values are those of the full program, operation for operation (keval_stat).
        // The full-program interpreter decodes every node for every element from LDS: 8 us per item
        // at n = 2049 against 4.  The aux tiles (y', the zero blocks, e_1') hold no covariance.
        by_shape(ntri, ntri, launch_split((long)ntri * p.n_fill_other));
        // (short jobs: chol_small_kernel takes y' from the observations and neither it nor
        // grad_kinv_small_kernel reads the zero blocks — one launch less in their chain)
        if (!small_job(g, Bc)) general(fill_lattice_kernel<true>, ntri, ntiles - ntri);
        break;
    case FILL_GRAD_FULL:
        general(fill_lattice_kernel<true>, off, ntiles - off);
        break;
    case FILL_VALUE_LISTS:   // Toeplitz jobs: single-table items store their diagonal tiles and aux rows
        // (the general kernel's split follows the chunk, not its share of it)
        by_shape(ntiles, g.toep ? ntiles - ntri + g.nb0 : ntiles, launch_split((long)ntiles * Bc));
        break;
    case FILL_VALUE_ONE:
        general(fill_lattice_kernel<false>, off, ntiles - off);
        break;
    }
}

// The product instantiation of the column sweep: NoProbe.  Weak, so that the diagnostic build
// (scripts/stamps/ngp_stamps.hip, linked beside this file into its own library) can put the
// stamping instantiation in their place; libngp.so contains these two and nothing of the probes.
// 1: chol_diag_wave_kernel (ngp_small_kernels.h), 0: chol_diag_kernel — a process-wide switch for
// same-box A/B runs (scripts/diag_form_ab.py), not part of the C-ABI
static std::atomic<int> g_diag_form{1};
extern "C" void ngp_debug_set_diag_form(int form) { g_diag_form.store(form); }

__attribute__((weak)) void launch_chol_diag(const JobGeom &g, const ChunkPtrs &p, int Bc, int j,
                                            int k0, hipStream_t s) {
    if (g_diag_form.load(std::memory_order_relaxed) && diag_wave(g, Bc))
        launch_chol_diag_wave(g, p, Bc, j, k0, s);
    else
        launch_chol_diag_t<NoProbe>(g, p, Bc, j, k0, s);
}

__attribute__((weak)) void launch_chol_col(const JobGeom &g, const ChunkPtrs &p, int Bc, int j,
                                           int mode, int k0, hipStream_t s, const DevSpec *sp) {
    launch_chol_col_t<NoProbe>(g, p, Bc, j, mode, k0, s, sp);
}

void launch_aux_back(const JobGeom &g, const ChunkPtrs &p, const double *dinv_all, size_t mstep,
                     double *Aout, int accumulate, int Bc, int c, hipStream_t s) {
    const int ntl = (g.naux + NB - 1) / NB;
    hipLaunchKernelGGL(aux_back_solve_kernel, dim3(ntl, Bc), dim3(256), 0, s, g, p,
                       dinv_all + (size_t)c * mstep, Aout, accumulate, c);
    if (c > 0) {
        const int ngrp = (c + 3) / 4;
        if (g.naux <= 16)
            hipLaunchKernelGGL(aux_back_update_kernel<1>, dim3(ntl * ngrp, Bc), dim3(256), 0, s, g,
                               p, c);
        else
            hipLaunchKernelGGL(aux_back_update_kernel<4>, dim3(ntl * ngrp, Bc), dim3(256), 0, s, g,
                               p, c);
    }
}

void launch_kapply(const JobGeom &g, const ChunkPtrs &p, const double *A, const double *X,
                   double *R, int Bc, const DevSpec &sp, hipStream_t s) {
    // accumulators per thread and column: 12 aux rows at a time (the usual d + m + 1 = 11 is one pass)
    constexpr int NACC = 12;
    const dim3 grid(g.nb0, Bc, (g.naux + NACC - 1) / NACC);   // 64 columns per workgroup (CPT = 1)
    if (g.lattice) {
        hipLaunchKernelGGL((kapply_kernel<NACC, 2, KA_SINGLE>), grid, dim3(256), 0, s, g, p, A, X, R,
                           sp);
        hipLaunchKernelGGL((kapply_kernel<NACC, 1, KA_REDUCED>), grid, dim3(256), 0, s, g, p, A, X,
                           R, sp);
        hipLaunchKernelGGL((kapply_kernel<NACC, 1, KA_CHAIN>), grid, dim3(256), 0, s, g, p, A, X, R,
                           sp);
    } else {
        hipLaunchKernelGGL((kapply_kernel<NACC, 1, KA_DIRECT>), grid, dim3(256), 0, s, g, p, A, X,
                           R, sp);
    }
}

void launch_refine_gram(const JobGeom &g, const double *A, const double *X, const double *R,
                        double *S, double *T, double *U, double *G, double *delta, int Bc,
                        const int32_t *items, hipStream_t s) {
    const int npairs = g.naux * g.naux;
    hipLaunchKernelGGL(refine_gram_pairs_kernel, dim3((npairs + 3) / 4, Bc), dim3(256), 0, s, g, A,
                       X, R, S, T, U, items);
    hipLaunchKernelGGL(refine_gram_final_kernel, dim3(Bc), dim3(256), 0, s, g, (const double *)S,
                       (const double *)T, (const double *)U, G, delta, items);
}

void launch_aux_update(const JobGeom &g, const ChunkPtrs &p, int Bc, int j, hipStream_t s) {
    const int n = (g.naux_pad / NB) * (g.nb0 - 1 - j);
    if (n <= 0) return;
    hipLaunchKernelGGL(aux_update_kernel, dim3((n + 3) / 4, Bc), dim3(256), 0, s, g, p, j);
}

bool launch_mixed_order(const ChunkPtrs &p, unsigned *prev, int32_t *order, int Bc, hipStream_t s) {
    // one workgroup ranks the chunk in LDS (4 B per item): chunks beyond NGP_MIXED_ORDER_MAX items
    // keep their dispatch order — with that many items a launch no longer ends on a few heavy
    // ones.  Returns whether `order` may be used (the launch was accepted).
    if (Bc > NGP_MIXED_ORDER_MAX) return false;
    (void)hipGetLastError();
    hipLaunchKernelGGL(mixed_order_kernel, dim3(1), dim3(256), sizeof(unsigned) * (size_t)Bc, s,
                       (const unsigned *)p.mixcnt, prev, order, Bc);
    return hipGetLastError() == hipSuccess;
}

void launch_diag_ahead(const JobGeom &g, const ChunkPtrs &p, int Bc, int j, hipStream_t s) {
    if (diag_ahead_waves(j) == 4)
        hipLaunchKernelGGL(diag_ahead_kernel<4>, dim3(Bc), dim3(256), 0, s, g, p, j);
    else
        hipLaunchKernelGGL(diag_ahead_kernel<1>, dim3(Bc), dim3(64), 0, s, g, p, j);
}

void launch_grad_kinv(const JobGeom &g, const double *L, double *Kinv, double *alpha, double *quad,
                      int Bc, hipStream_t s, hipStream_t side, hipEvent_t fork, hipEvent_t join) {
    // long series (2 x 2 tile blocks staged through LDS): alpha = W_I z comes out of the K^-1 kernel
    // itself, from the rows it stages; the alpha kernel is left with the quadratic form z'z (one
    // wave per item).  Shorter series: alpha reads every row of W once and does not depend on K^-1:
    // it runs beside it on the side stream.
    const bool lds = kinv_lds(g);
    const int a_first = lds ? g.n0 : 0;
    const dim3 agrid(lds ? 1 : (g.n0 + 1 + 3) / 4, Bc);
    const bool beside = side && fork && join;
    if (beside) {
        (void)hipEventRecord(fork, s);
        (void)hipStreamWaitEvent(side, fork, 0);
        hipLaunchKernelGGL(grad_alpha_kernel, agrid, dim3(256), 0, side, g, L, alpha, quad, a_first);
        (void)hipEventRecord(join, side);
    }
    const int npairs = g.nb0 * (g.nb0 + 1) / 2;
    if (lds) {   // HBM traffic halves against the wave-per-tile form
        const int nb2 = (g.nb0 + 1) / 2, nblk = nb2 * (nb2 + 1) / 2;
        hipLaunchKernelGGL(grad_kinv_lds_kernel, dim3(nblk * ((Bc + 7) / 8 * 8)), dim3(256), 0, s, g, L,
                           Kinv, nblk, Bc, alpha);
    } else {
        hipLaunchKernelGGL(grad_kinv_kernel, dim3((npairs + 3) / 4, Bc), dim3(256), 0, s, g, L, Kinv,
                           npairs);
    }
    if (beside)
        (void)hipStreamWaitEvent(s, join, 0);
    else
        hipLaunchKernelGGL(grad_alpha_kernel, agrid, dim3(256), 0, s, g, L, alpha, quad, a_first);
}

void launch_grad_contract(const JobGeom &g, const ChunkPtrs &p, const double *Kinv,
                          const double *alpha, const double *quad, double *partials, double *grad,
                          double *logml, int Bc, const DevSpec &sp, hipStream_t s0,
                          const int32_t *items, const int32_t *bucket_counts, hipStream_t side,
                          hipEvent_t fork, hipEvent_t join) {
    const int ntri = g.nb0 * (g.nb0 + 1) / 2;
    int nparts = ntri;
    const bool two = side && fork && join && items && contract_two_streams(Bc);
    int nlaunched = 0;
    hipStream_t s = s0;
    if (two) {
        (void)hipEventRecord(fork, s0);
        (void)hipStreamWaitEvent(side, fork, 0);
    }
    if (g.lattice && p.dtab) {
        const int split = grad_contract_split(ntri, Bc, g.invariant != 0);
        // items sorted by tree size (grad_bucket): 1, 2, 4, 8 leaves on the register-accumulator
        // kernel, up to 16 leaves in two passes of it, larger trees on the general kernel
        const int32_t *it = items;
        int32_t whole[GRAD_BUCKETS] = {};
        whole[grad_bucket(g.maxops)] = Bc;
        const int32_t *cnt = items ? bucket_counts : whole;
        const int tpw = contract_tiles_per_wg(g, split, ntri, Bc, cnt[GRAD_BUCKETS - 1] != 0);
        const int ngrp = (ntri + tpw - 1) / tpw;
        nparts = ngrp * split;
        for (int bk = 0; bk < GRAD_BUCKETS; ++bk) {
            const int nb = cnt[bk];
            if (nb <= 0) continue;
            s = (two && (nlaunched++ & 1)) ? side : s0;
            const dim3 grid(ngrp * split, nb), blk(256);
#define NGP_LAUNCH_LISTS(...)                                                                    \
    hipLaunchKernelGGL((grad_contract_lists_kernel<__VA_ARGS__>), grid, blk, 0, s, g, p, Kinv, alpha, \
                       partials, ntri, split, sp, it, tpw)
            if (bk == 0) NGP_LAUNCH_LISTS(1);
            else if (bk == 1) NGP_LAUNCH_LISTS(2);
            else if (bk == 2) NGP_LAUNCH_LISTS(4);
            else if (bk == 3) NGP_LAUNCH_LISTS(8);
            else if (bk == 4) {   // 9 .. 16 leaves: two passes of eight accumulator sets
                NGP_LAUNCH_LISTS(16, 8, 0);
                NGP_LAUNCH_LISTS(16, 8, 1);
            } else if (g.maxops <= LDSV_OPS)
                hipLaunchKernelGGL(grad_contract_lattice_kernel<true>, grid, blk, 0, s, g, p, Kinv,
                                   alpha, partials, ntri, split, sp, it);
            else
                hipLaunchKernelGGL(grad_contract_lattice_kernel<false>, grid, blk, 0, s, g, p, Kinv,
                                   alpha, partials, ntri, split, sp, it);
#undef NGP_LAUNCH_LISTS
            if (it) it += nb;
        }
    } else {
        hipLaunchKernelGGL(grad_contract_kernel, dim3(ntri, Bc), dim3(256), 0, s0, g, p.progs, p.t0,
                           Kinv, alpha, partials, ntri, sp);
    }
    if (two) {
        (void)hipEventRecord(join, side);
        (void)hipStreamWaitEvent(s0, join, 0);
    }
    hipLaunchKernelGGL(grad_reduce_kernel, dim3(Bc), dim3(128), 0, s0, g, p.progs, partials, quad,
                       p.logdet, grad, logml, nparts);
}

// The Toeplitz gradient path after the factorisation and the backward sweep: weights per distance
// from A = [a' ; x'], then the 1-D contraction (DIAG instantiations, by tree-size bucket) and the
// final sum.  items / bucket_counts as in launch_grad_contract (null: one launch sized by maxops).
void launch_toep_grad(const JobGeom &g, const ChunkPtrs &p, const double *A, double *wbuf,
                      const double *quad, double *partials, double *grad, double *logml, int Bc,
                      const DevSpec &sp, hipStream_t s, const int32_t *items,
                      const int32_t *bucket_counts) {
    const int nd = (g.n_real + 255) / 256;
    const size_t lds = sizeof(double) * (2 * (size_t)g.n_real + 1);   // <= 128 KiB: n <= 8192 (ngp_grad_stage)
    if (lds > 48 * 1024)
        (void)hipFuncSetAttribute((const void *)toep_weights_kernel,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(toep_weights_kernel, dim3(nd, Bc), dim3(256), lds, s, g, A, wbuf);
    int32_t whole[GRAD_BUCKETS] = {};
    whole[grad_bucket(g.maxops)] = Bc;
    const int32_t *cnt = items ? bucket_counts : whole;
    const int32_t *it = items;
    for (int bk = 0; bk < GRAD_BUCKETS; ++bk) {
        const int nb = cnt[bk];
        if (nb <= 0) continue;
        const dim3 grid(nd, nb), blk(256);
#define NGP_LAUNCH_DIAG(...)                                                                     \
    hipLaunchKernelGGL((grad_contract_lists_kernel<__VA_ARGS__, true>), grid, blk, 0, s, g, p, wbuf, \
                       wbuf, partials, nd, 1, sp, it)
        if (bk == 0) NGP_LAUNCH_DIAG(1, 1, 0);
        else if (bk == 1) NGP_LAUNCH_DIAG(2, 2, 0);
        else if (bk == 2) NGP_LAUNCH_DIAG(4, 4, 0);
        else if (bk == 3) NGP_LAUNCH_DIAG(8, 8, 0);
        else {   // 9 .. 32 leaves: passes of eight accumulator sets (NGP_MAX_OPS = 64 nodes)
            NGP_LAUNCH_DIAG(16, 8, 0);
            NGP_LAUNCH_DIAG(16, 8, 1);
        }
#undef NGP_LAUNCH_DIAG
        if (it) it += nb;
    }
    hipLaunchKernelGGL(grad_reduce_kernel, dim3(Bc), dim3(128), 0, s, g, p.progs, partials, quad,
                       p.logdet, grad, logml, nd);
}

void launch_toep_quad(const JobGeom &g, const double *L, double *quad, int Bc, hipStream_t s) {
    hipLaunchKernelGGL(toep_quad_kernel, dim3(Bc), dim3(256), 0, s, g, L, quad);
}

void launch_gram(const JobGeom &g, const double *L, double *G, int Bc, hipStream_t s) {
    if (g.n0 == 0) return;
    hipLaunchKernelGGL(gram_kernel, dim3(Bc), dim3(256), 0, s, g, L, G);
}

void launch_epilogue(const JobGeom &g, const EpiPtrs &p, const DevSpec &sp, hipStream_t s) {
    const size_t bytes = 8 * ((size_t)g.da * g.da + (size_t)g.m * g.da + (size_t)g.da);
    const int lds_work = bytes > 0 && bytes <= 60 * 1024;
    hipLaunchKernelGGL(epilogue_kernel, dim3(g.B), dim3(64), lds_work ? bytes : 0, s, g, p, sp,
                       lds_work);
}

void launch_component_fill(const JobGeom &g, const ChunkPtrs &p, const CompPtrs &cp, int Bc,
                           const DevSpec &sp, hipStream_t s) {
    if (g.n0 == 0) return;
    const int mt = (cp.m + NB - 1) / NB;
    hipLaunchKernelGGL(component_fill_kernel, dim3(g.nb0 * mt, Bc, cp.cmax), dim3(256), 0, s, g, p, cp,
                       sp);
}

void launch_component_epilogue(const JobGeom &g, const EpiPtrs &p, const CompPtrs &cp,
                               const DevSpec &sp, hipStream_t s) {
    const size_t bytes = sizeof(double) * (size_t)comp_epi_small(g.da);
    const int lds_work = bytes <= (size_t)COMP_EPI_LDS_BYTES;
    hipLaunchKernelGGL(component_epilogue_kernel, dim3(g.B), dim3(64), lds_work ? bytes : 0, s, g, p,
                       cp, sp, lds_work);
}

void launch_cov(const DevProgram *progs, int B, const double *t1, int n1, const double *t2, int n2,
                int add_diag, double *out, const DevSpec &sp, hipStream_t s) {
    long total = (long)n1 * n2;
    int gx = (int)((total + 255) / 256);
    if (gx > 2048) gx = 2048;
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(cov_kernel, dim3(gx, B), dim3(256), 0, s, progs, t1, n1, t2, n2, add_diag,
                       out, sp);
}

// the workgroups of a long-horizon kernel whose threads stride over `total` elements
static int long_blocks(long total) { return (int)std::max<long>(1, std::min<long>(4096, (total + 255) / 256)); }

void launch_long(int step, const LongGeom &g, const LongPtrs &p, const DevSpec &sp, hipStream_t s) {
    const int nt = g.qpad / NB, ct = g.c / NB + 1;
    const long small = (long)g.q1 * (g.c + 2) + (g.want_sigma ? (long)g.m * g.m : 0);
    switch (step) {
    case LONG_FILL:
        if (g.n0 == 0) return;
        hipLaunchKernelGGL(long_fill_kernel, dim3(long_blocks((long)g.qpad * g.n0), g.B), dim3(256), 0, s, g, p, sp);
        return;
    case LONG_SMALL:
        hipLaunchKernelGGL(long_small_kernel, dim3(long_blocks(small), g.B), dim3(256), 0, s, g, p, sp);
        return;
    case LONG_SOLVE:
        if (g.n0 == 0) return;
        hipLaunchKernelGGL(long_solve_kernel, dim3((g.qpad + LONG_WG_TILE - 1) / LONG_WG_TILE, g.B),
                           dim3(256), 0, s, g, p);
        return;
    case LONG_GRAM: {
        if (g.n0 == 0) return;
        const int npairs = g.want_sigma ? nt * (nt + 1) / 2 : ct * nt + (nt - ct);
        hipLaunchKernelGGL(long_gram_kernel, dim3((npairs + 3) / 4, g.B), dim3(256), 0, s, g, p, npairs);
        return;
    }
    case LONG_COND:
        hipLaunchKernelGGL(long_cond_kernel, dim3(g.B), dim3(256),
                           g.c <= LONG_COND_LDS ? 8 * (size_t)g.c * g.c : 0, s, g, p);
        return;
    case LONG_APPLY:
        hipLaunchKernelGGL(long_apply_kernel, dim3((g.m + 63) / 64, g.B), dim3(64), 0, s, g, p, sp);
        return;
    case LONG_SIGMA:
        if (!g.want_sigma) return;
        hipLaunchKernelGGL(long_sigma_kernel, dim3(long_blocks((long)g.m * g.m), g.B), dim3(256), 0, s, g, p, sp);
        return;
    }
}

void launch_long_comp(int step, const LongGeom &g, const LongPtrs &p, const LongCompGeom &cg,
                      const LongCompPtrs &cp, const DevSpec &sp, hipStream_t s) {
    const int nt = g.qpad / NB, ht = cg.hpad / NB, mt = cg.mpad / NB, groups = 1 + cg.cmax;
    const int gpairs = cg.cmax * (cg.cmax + 1) / 2;
    const long wid = (long)cg.cmax * cg.m;
    switch (step) {
    case LCOMP_FILL:
        if (g.n0 == 0) return;
        hipLaunchKernelGGL(lcomp_fill_kernel, dim3(long_blocks((long)std::max(cg.hpad, cg.mpad) * g.n0), g.B, groups),
                           dim3(256), 0, s, g, p, cg, cp, sp);
        return;
    case LCOMP_SMALL:
        hipLaunchKernelGGL(lcomp_small_kernel,
                           dim3(long_blocks(std::max<long>((long)cg.hpad * (g.c + 1),
                                                      (long)cg.m * (g.c + 2 + cg.cmax + (g.want_sigma ? wid : 0)))),
                                g.B, groups),
                           dim3(256), 0, s, g, p, cg, cp, sp);
        return;
    case LCOMP_GRAM: {
        if (g.n0 == 0) return;
        const int npairs = g.want_sigma ? nt * (nt + 1) / 2 : ht * nt + gpairs * mt;
        hipLaunchKernelGGL(lcomp_gram_kernel, dim3((npairs + 3) / 4, g.B), dim3(256), 0, s, g, p, cg, cp, npairs);
        return;
    }
    case LCOMP_APPLY:
        hipLaunchKernelGGL(lcomp_apply_kernel, dim3((cg.m + 63) / 64, g.B, cg.cmax), dim3(64), 0, s, g, p, cg, cp);
        return;
    case LCOMP_CROSS:
        hipLaunchKernelGGL(lcomp_cross_kernel, dim3((cg.m + 63) / 64, g.B, std::min(gpairs, 65535)), dim3(64), 0, s,
                           g, p, cg, cp);
        return;
    case LCOMP_SIGMA:
        if (!g.want_sigma) return;
        hipLaunchKernelGGL(lcomp_sigma_kernel, dim3(long_blocks(wid * wid), g.B), dim3(256), 0, s, g, p, cg, cp);
        return;
    }
}

void launch_long_origin(int step, const LongGeom &g, const LongPtrs &p, const LongOriginGeom &og,
                        const LongOriginPtrs &op, const DevSpec &sp, hipStream_t s) {
    switch (step) {
    case LORG_MAIN:
        if (g.n0 == 0 || og.R0 == 0) return;
        hipLaunchKernelGGL(lorg_main_kernel, dim3((g.m + 63) / 64, g.B), dim3(64), 0, s, g, p, og, op, sp);
        return;
    case LORG_TAIL:
        hipLaunchKernelGGL(lorg_tail_kernel, dim3((g.m + 63) / 64, g.B), dim3(64), 0, s, g, p, og, op, sp);
        return;
    case LORG_LOGML:
        if (!op.logml) return;
        hipLaunchKernelGGL(lorg_logml_kernel, dim3(g.B), dim3(256), 0, s, g, p, og, op);
        return;
    }
}

void launch_mfma_bench(double *out, int iters, int blocks, hipStream_t s) {
    hipLaunchKernelGGL(mfma_bench_kernel, dim3(blocks), dim3(256), 0, s, out, iters);
}
void launch_mfma_bench_detail(unsigned long long *stamps, int iters, int blocks, hipStream_t s) {
    hipLaunchKernelGGL(mfma_bench_detail_kernel, dim3(blocks), dim3(256), 0, s, stamps, iters);
}
void launch_mfma_layout_probe(const double *A, const double *Bm, double *Dout, hipStream_t s) {
    hipLaunchKernelGGL(mfma_layout_probe_kernel, dim3(1), dim3(64), 0, s, A, Bm, Dout);
    hipLaunchKernelGGL(mfma4_composite_probe_kernel, dim3(1), dim3(64), 0, s, A, Bm, Dout + 256);
}
void launch_mfma_f32_probe(const float *A, const float *Bm, float *Dout, hipStream_t s) {
    hipLaunchKernelGGL(mfma_f32_probe_kernel, dim3(1), dim3(64), 0, s, A, Bm, Dout);
}
void launch_stream_write(double *dst, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(stream_write_kernel, dim3(2048), dim3(256), 0, s,
                       reinterpret_cast<f64x2 *>(dst), (long)(n / 2));
}
void launch_stream_copy(double *dst, const double *src, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(stream_copy_kernel, dim3(2048), dim3(256), 0, s,
                       reinterpret_cast<f64x2 *>(dst), reinterpret_cast<const f64x2 *>(src),
                       (long)(n / 2));
}

}  // namespace ngp

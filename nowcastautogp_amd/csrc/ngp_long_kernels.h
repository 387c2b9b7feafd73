// ngp_long_kernels.h — ngp_factor_predict_long: a forecast horizon of up to NGP_MAX_LONG_HORIZON
// dates from the resident factor in one query.  Included from
// ngp_kernels.hip behind ngp_col_kernels.h and ngp_tree_kernels.h.
//
// The dates do not travel as aux rows of the factorisation: they are the right-hand-side panel of a
// triangular solve against the resident L.  Per item the panel is stored row per panel column,
//     W [qpad x n0]:  row 0 = y0',  rows 1 .. c = k(tail and appended points, t0),
//                     rows c + 1 .. c + m = k(dates, t0),  zero rows up to a multiple of 64
// which is the layout of the aux rows, so the tile product (gemm_rows) and the 64-wide solve on the
// accumulators (solve_and_store_lds) of the column kernels are used as they are.
//
//   long_fill_kernel    the panel, through keval (ngp_tree_kernels.h)
//   long_small_kernel   k over [tail, appended, dates]: S (q1 x (c + 1)), the dates' diagonal, and
//                       the lower triangle of the m x m block when sigma is asked for
//   long_solve_kernel   W <- W L^-T, left-looking over the block columns: one wave per LONG_TILE
//                       panel columns, four waves (LONG_WG_TILE columns) share the rows of L and M_j
//   long_gram_kernel    S, diagonal and m x m block minus the products of rows of W (fp64 MFMA, one
//                       64 x 64 tile pair per wave, k ascending: the same bits whichever launch
//                       shape asks for an element)
//   long_cond_kernel    S_cc = G G' in place (first non-positive pivot reported), u_s = G^-1 e_s
//   long_apply_kernel   one date per thread: its row of W = S_mc G^-T, mean per scenario, variance
//   long_sigma_kernel   Sigma = S_mm - W W', lower triangle computed, mirrored on store
#pragma once
#include "ngp_internal.h"
#include "ngp_mfma.h"

namespace ngp {

__global__ __launch_bounds__(256) void long_fill_kernel(LongGeom g, LongPtrs p, DevSpec sp) {
    __shared__ DevProgram P;
    const int item = blockIdx.y;
    load_program(&P, p.progs + item);
    __syncthreads();
    const long total = (long)g.qpad * g.n0;
    double *W = p.W + (long)item * total;
    const double *y0 = p.y0 + (g.y_shared ? 0 : (long)item * g.n0);
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int r = (int)(e / g.n0), k = (int)(e % g.n0);
        double v = 0.0;
        if (r == 0) v = y0[k];
        else if (r < g.q1) v = keval(P, sp, p.tp[r - 1], p.t0[k]);
        W[e] = v;
    }
}

// S [q1][cw]: column 0 belongs to y' (left zero here), column j >= 1 to conditioning point j;
// row r >= 1 to panel row r.  Only r >= j is read later.
__global__ __launch_bounds__(256) void long_small_kernel(LongGeom g, LongPtrs p, DevSpec sp) {
    __shared__ DevProgram P;
    const int item = blockIdx.y;
    load_program(&P, p.progs + item);
    __syncthreads();
    const double nz = P.noise + sp.jitter;
    const int cw = g.c + 1;
    const long nS = (long)g.q1 * cw, nD = g.q1, nG = g.want_sigma ? (long)g.m * g.m : 0;
    double *S = p.S + (long)item * nS;
    double *dg = p.dg + (long)item * nD;
    double *Sg = g.want_sigma ? p.sigma + (long)item * g.sig_stride : nullptr;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < nS + nD + nG; e += (long)gridDim.x * 256) {
        if (e < nS) {
            const int r = (int)(e / cw), j = (int)(e % cw);
            double v = 0.0;
            if (j >= 1 && r >= j) {
                v = keval(P, sp, p.tp[r - 1], p.tp[j - 1]);
                if (r == j) v += nz;
            }
            S[e] = v;
        } else if (e < nS + nD) {
            const int r = (int)(e - nS);
            dg[r] = r > g.c ? keval(P, sp, p.tp[r - 1], p.tp[r - 1]) : 0.0;
        } else {
            const long x = e - nS - nD;
            const int i = (int)(x / g.m), j = (int)(x % g.m);
            if (j <= i) Sg[(long)i * g.sig_ld + j] = keval(P, sp, p.tp[g.c + i], p.tp[g.c + j]);
        }
    }
}

// W_j = (X_j - sum_{k < j} W_k L_jk') M_j' for j = 0 .. nb0 - 1 inside one launch.  A wave owns its
// LONG_TILE rows of W for the whole sweep and reads back only what it has written itself; block row
// j of L is read as full rows, k ascending, once per workgroup tile.
__global__ __launch_bounds__(256, 1) void long_solve_kernel(LongGeom g, LongPtrs p) {
    __shared__ __attribute__((aligned(16))) char epi[EPI_LDS_BYTES];
    const int item = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = blockIdx.x * (LONG_WG_TILE / LONG_TILE) + wave;
    const bool valid = tile * LONG_TILE < g.q1;    // wave-uniform; qpad covers every valid tile
    const long ld = g.ld;
    const double *Lit = p.L + (long)item * g.L_stride;
    double *Wr = p.W + ((long)item * g.qpad + (long)(valid ? tile : 0) * LONG_TILE) * ld;
    const int r16 = lane & 15, q = lane >> 4;
    const double *pb = Wr + (long)r16 * ld + 2 * q;
    double *lds_m = reinterpret_cast<double *>(epi);
    double *buf = reinterpret_cast<double *>(epi + EPI_M_BYTES + wave * EPI_WAVE_BYTES);
    NoProbe probe;
    for (int j = 0; j < g.nb0; ++j) {
        double acc4[4][4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc4[a][b][r] = 0.0;
        const int kmax = j * NB;
        const double *pa = Lit + ((long)j * NB + r16) * ld + 2 * q;
        if (valid) gemm_rows<4>(acc4, pa, pb, ld, 0, kmax);
        __syncthreads();                           // every wave is done with M of the step before
        stage_mstrips(lds_m, p.dinv + (long)j * g.dinv_step + (long)item * (NB * NB), tid);
        __syncthreads();
        if (valid)
            solve_and_store_lds(acc4, Wr, lds_m, ld, kmax, lane, buf, probe);
        __threadfence_block();                     // the wave's own rows, before it reads them back
    }
}

// pair -> (ta, tb), ta >= tb.  want_sigma: every pair of the lower triangle; else the ct tile
// columns that hold y' and the conditioning rows, then the diagonal tiles behind them.
__device__ __forceinline__ bool long_pair_of(const LongGeom &g, int pair, int &ta, int &tb) {
    const int nt = g.qpad / NB, ct = g.c / NB + 1;
    if (g.want_sigma) {
        tri_decode(pair, ta, tb);
        return ta < nt;
    }
    if (pair < ct * nt) {
        tb = pair / nt;
        ta = pair % nt;
        return ta >= tb;
    }
    ta = tb = ct + (pair - ct * nt);
    return ta < nt;
}

__global__ __launch_bounds__(256, 1) void long_gram_kernel(LongGeom g, LongPtrs p, int npairs) {
    const int item = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pair = blockIdx.x * 4 + wave;
    if (pair >= npairs) return;
    int ta, tb;
    if (!long_pair_of(g, pair, ta, tb)) return;
    const long ld = g.ld;
    const double *W = p.W + (long)item * g.qpad * ld;
    const int r16 = lane & 15, q = lane >> 4;
    double acc4[4][4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc4[a][b][r] = 0.0;
    gemm_rows<4>(acc4, W + ((long)ta * NB + r16) * ld + 2 * q, W + ((long)tb * NB + r16) * ld + 2 * q,
                 ld, 0, g.n0);
    const int cw = g.c + 1;
    double *S = p.S + (long)item * g.q1 * cw;
    double *dg = p.dg + (long)item * g.q1;
    double *Sg = g.want_sigma ? p.sigma + (long)item * g.sig_stride : nullptr;
    const int n16 = lane & 15, isub = lane >> 4;
    const int jj0 = 4 * (n16 >> 2) + isub;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int it = 0; it < 4; ++it)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ra = ta * NB + 16 * jt + jj0;                       // row of the A operand
                const int rb = tb * NB + 16 * it + ((n16 + 4 * r) & 15);      // row of the B operand
                if (ra >= g.q1 || rb > ra) continue;
                const double v = acc4[jt][it][r];
                if (rb == 0) S[(long)ra * cw] = v;
                else if (rb <= g.c) S[(long)ra * cw + rb] -= v;
                if (ra == rb && ra > g.c) dg[ra] -= v;
                if (Sg && rb > g.c) Sg[(long)(ra - g.c - 1) * g.sig_ld + (rb - g.c - 1)] -= v;
            }
}

// LONG_COND_LDS: the largest c whose c x c block is factorised in LDS; beyond, in place in S
constexpr int LONG_COND_LDS = 88;
__global__ __launch_bounds__(256) void long_cond_kernel(LongGeom g, LongPtrs p) {
    extern __shared__ double long_dyn[];
    __shared__ int bad;
    const int item = blockIdx.x, tid = threadIdx.x;
    const int c = g.c, cw = c + 1;
    const int finfo = p.finfo ? p.finfo[item] : 0;   // no main block: create had nothing to report
    if (finfo > 0 || c == 0) {
        if (tid == 0) p.info[item] = finfo;
        return;
    }
    if (tid == 0) bad = 0;
    double *S = p.S + (long)item * g.q1 * cw;
    double *Sc = S + cw + 1;                      // S_cc: element (a, b) at Sc[a * cw + b]
    const bool in_lds = c <= LONG_COND_LDS;
    double *A = in_lds ? long_dyn : Sc;
    const int lda = in_lds ? c : cw;
    if (in_lds)
        for (int e = tid; e < c * c; e += 256) A[e] = Sc[(e / c) * cw + e % c];
    __syncthreads();
    for (int k = 0; k < c; ++k) {                 // right-looking, a row per thread
        const double akk = A[k * lda + k];
        const double dk = sqrt(akk);
        __syncthreads();
        if (tid == 0) {
            if (!(akk > 0.0) && bad == 0) bad = k + 1;
            A[k * lda + k] = dk;
        }
        for (int i = k + 1 + tid; i < c; i += 256) A[i * lda + k] /= dk;
        __syncthreads();
        for (int i = k + 1 + tid; i < c; i += 256) {
            const double lik = A[i * lda + k];
            for (int jj = k + 1; jj <= i; ++jj) A[i * lda + jj] -= lik * A[jj * lda + k];
        }
        __syncthreads();
    }
    if (in_lds) {
        for (int e = tid; e < c * c; e += 256) Sc[(e / c) * cw + e % c] = A[e];
        __syncthreads();
    }
    // u_s = G^-1 (y_c,s - V_c' v_y): a scenario per thread
    const double *yc = p.yc + (g.y_shared ? 0 : (long)item * g.D * c);
    for (int s = tid; s < g.D; s += 256) {
        double *z = p.z + ((long)item * g.D + s) * c;
        for (int a = 0; a < c; ++a) {
            double e = yc[(long)s * c + a] - S[(long)(1 + a) * cw];
            for (int pp = 0; pp < a; ++pp) e -= Sc[a * cw + pp] * z[pp];
            z[a] = e / Sc[a * cw + a];
        }
    }
    if (tid == 0) p.info[item] = bad ? g.n0 + bad : finfo;
}

// s - sum_a wi[a] wj[a], a ascending: the variance and the diagonal of sigma go through this one
// expression, so they agree bit for bit
__device__ __forceinline__ double long_schur_sub(double s, const double *wi, const double *wj, int c) {
    for (int a = 0; a < c; ++a) s = fma(-wi[a], wj[a], s);
    return s;
}

__global__ __launch_bounds__(64) void long_apply_kernel(LongGeom g, LongPtrs p, DevSpec sp) {
    const int item = blockIdx.y;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= g.m) return;
    const int c = g.c, cw = c + 1, r = c + 1 + i;
    double *mu = p.mu + (long)item * g.D * g.m;
    double *var = p.var + (long)item * g.m;
    if (p.info[item] > 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        for (int s = 0; s < g.D; ++s) mu[(long)s * g.m + i] = nan;
        var[i] = nan;
        return;
    }
    double *S = p.S + (long)item * g.q1 * cw;
    const double *Sc = S + cw + 1;
    double *w = S + (long)r * cw + 1;             // the date's row of S_mc, then of W
    for (int a = 0; a < c; ++a) {
        double s = w[a];
        for (int pp = 0; pp < a; ++pp) s -= w[pp] * Sc[a * cw + pp];
        w[a] = s / Sc[a * cw + a];
    }
    double v = long_schur_sub(p.dg[(long)item * g.q1 + r], w, w, c);
    if (g.noise_on_new) v += p.progs[item].noise + sp.jitter;
    var[i] = v;
    const double mu0 = g.n0 ? S[(long)r * cw] : 0.0;
    for (int s = 0; s < g.D; ++s) {
        const double *z = p.z + ((long)item * g.D + s) * c;
        double x = mu0;
        for (int a = 0; a < c; ++a) x += w[a] * z[a];
        mu[(long)s * g.m + i] = x;
    }
}

__global__ __launch_bounds__(256) void long_sigma_kernel(LongGeom g, LongPtrs p, DevSpec sp) {
    const int item = blockIdx.y;
    const int c = g.c, cw = c + 1;
    const long total = (long)g.m * g.m;
    double *Sg = p.sigma + (long)item * g.sig_stride;
    const double *S = p.S + (long)item * g.q1 * cw;
    const bool failed = p.info[item] > 0;
    const double nz = p.progs[item].noise + sp.jitter;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int i = (int)(e / g.m), j = (int)(e % g.m);
        if (j > i) continue;
        double s;
        if (failed) {
            s = __longlong_as_double(0x7ff8000000000000LL);
        } else {
            s = long_schur_sub(Sg[(long)i * g.sig_ld + j], S + (long)(c + 1 + i) * cw + 1, S + (long)(c + 1 + j) * cw + 1, c);
            if (i == j && g.noise_on_new) s += nz;
        }
        Sg[(long)i * g.sig_ld + j] = s;
        Sg[(long)j * g.sig_ld + i] = s;
    }
}

}  // namespace ngp

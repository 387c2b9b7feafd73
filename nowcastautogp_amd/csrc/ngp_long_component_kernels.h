// ngp_long_component_kernels.h — ngp_factor_components_long: the additive decomposition of a forecast
// over a horizon of up to NGP_MAX_LONG_HORIZON dates in one query.  Included
// from ngp_kernels.hip behind ngp_long_kernels.h, whose solve (long_solve_kernel), conditioning
// block (long_cond_kernel) and long_schur_sub are used as they are.
//
// The panel of an item is the long query's with the date rows replaced by cmax groups of date rows:
//     W [qpad x n0]:  row 0 = y0',  rows 1 .. c = k(tail and appended points, t0),  zero up to hpad,
//                     rows hpad + g mpad + i = k_g(date i, t0),  i < m,  zero up to mpad
// hpad and mpad are multiples of 64, so date i of every group sits at the same place of its 64-row
// tile and the same-date covariances of two parts are the diagonals of aligned tile pairs.  S has a
// row per panel row: S [qpad][c + 1], column 0 = the row's product with y', column j >= 1 the
// conditioning point j.  An item with fewer than cmax components leaves its last groups zero.
//
//   lcomp_fill_kernel   the panel; a workgroup's row group, hence its program, is uniform
//   lcomp_small_kernel  k over the conditioning points, k_g(dates, conditioning points), the prior
//                       delta_gg' k_g(t*, t*): its same-date entries into cross, the lower triangle
//                       of the blocks into sigma when sigma is asked for
//   lcomp_gram_kernel   the products of solved rows: every row x the conditioning columns, the
//                       same-date tile pairs across groups, every tile pair when sigma is asked for
//                       (fp64 MFMA, one 64 x 64 tile pair per wave, k ascending: the same bits
//                       whichever launch shape asks for an element)
//   lcomp_apply_kernel  one (date, group) per thread: its row of S_mc G^-T, the mean per scenario
//   lcomp_cross_kernel  one (date, pair of groups) per thread: cross, mirrored on store
//   lcomp_sigma_kernel  sigma: lower triangle computed, mirrored on store
#pragma once
#include "ngp_internal.h"
#include "ngp_mfma.h"

namespace ngp {

// the components of an item: its first program / output row in the chunk and their number
__device__ __forceinline__ int lcomp_first(const LongCompPtrs &cp, int item) { return cp.first[item] - cp.first[0]; }
__device__ __forceinline__ int lcomp_count(const LongCompPtrs &cp, int item) { return cp.first[item + 1] - cp.first[item]; }

// blockIdx.z: 0 = y' and the conditioning rows under the item's own program, 1 + g = group g
__global__ __launch_bounds__(256) void lcomp_fill_kernel(LongGeom g, LongPtrs p, LongCompGeom cg,
                                                         LongCompPtrs cp, DevSpec sp) {
    __shared__ DevProgram P;
    const int item = blockIdx.y, grp = (int)blockIdx.z - 1;
    const bool live = grp < lcomp_count(cp, item);
    if (live) load_program(&P, grp < 0 ? p.progs + item : cp.progs + lcomp_first(cp, item) + grp);
    __syncthreads();
    const int row0 = grp < 0 ? 0 : cg.hpad + grp * cg.mpad;
    const int rows = grp < 0 ? cg.hpad : cg.mpad;
    const int nlive = !live ? 0 : grp < 0 ? 1 + g.c : cg.m;
    const int tp0 = grp < 0 ? -1 : g.c;            // tp index of the group's row 0
    const long total = (long)rows * g.n0;
    double *W = p.W + ((long)item * g.qpad + row0) * g.n0;
    const double *y0 = p.y0 + (g.y_shared ? 0 : (long)item * g.n0);
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int r = (int)(e / g.n0), k = (int)(e % g.n0);
        double v = 0.0;
        if (r < nlive) v = (grp < 0 && r == 0) ? y0[k] : keval(P, sp, p.tp[tp0 + r], p.t0[k]);
        W[e] = v;
    }
}

// Head (blockIdx.z = 0): S of y' and the conditioning rows as long_small_kernel leaves it.  Group g:
// its rows of S; the prior's same-date entries cross[g][g'][i], g' <= g (k_g(t_i, t_i) for g' = g,
// else 0); with sigma rows g m + i of the item's block, columns up to the diagonal.
__global__ __launch_bounds__(256) void lcomp_small_kernel(LongGeom g, LongPtrs p, LongCompGeom cg,
                                                          LongCompPtrs cp, DevSpec sp) {
    __shared__ DevProgram P;
    const int item = blockIdx.y, grp = (int)blockIdx.z - 1;
    const int nc = lcomp_count(cp, item);
    if (grp >= nc) return;                         // uniform over the workgroup
    load_program(&P, grp < 0 ? p.progs + item : cp.progs + lcomp_first(cp, item) + grp);
    __syncthreads();
    const int cw = g.c + 1, m = cg.m;
    double *S = p.S + (long)item * g.q1 * cw;
    if (grp < 0) {
        const double nz = P.noise + sp.jitter;
        const long nS = (long)cg.hpad * cw;
        for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < nS; e += (long)gridDim.x * 256) {
            const int r = (int)(e / cw), j = (int)(e % cw);
            double v = 0.0;
            if (j >= 1 && r >= j && r <= g.c) {
                v = keval(P, sp, p.tp[r - 1], p.tp[j - 1]);
                if (r == j) v += nz;
            }
            S[e] = v;
        }
        return;
    }
    const double *td = p.tp + g.c;                 // the dates
    double *Sr = S + (long)(cg.hpad + grp * cg.mpad) * cw;
    double *cr = cp.cross + (cp.cr_off[item] - cp.cr_off[0]) * m + (long)grp * nc * m;
    const long CM = (long)nc * m, wid = (long)(grp + 1) * m;
    double *Sg = g.want_sigma ? cp.sigma + (cp.sig_off[item] - cp.sig_off[0]) + (long)grp * m * CM : nullptr;
    const long nS = (long)m * cw, nC = wid, nG = g.want_sigma ? (long)m * wid : 0;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < nS + nC + nG; e += (long)gridDim.x * 256) {
        if (e < nS) {
            const int i = (int)(e / cw), j = (int)(e % cw);
            Sr[e] = j >= 1 ? keval(P, sp, td[i], p.tp[j - 1]) : 0.0;
        } else if (e < nS + nC) {
            const long x = e - nS;
            const int g2 = (int)(x / m), i = (int)(x % m);
            cr[x] = g2 == grp ? keval(P, sp, td[i], td[i]) : 0.0;
        } else {
            const long x = e - nS - nC;
            const int i = (int)(x / wid);
            const long J = x % wid;
            const int g2 = (int)(J / m), j = (int)(J % m);
            if (g2 < grp) Sg[(long)i * CM + J] = 0.0;
            else if (j <= i) Sg[(long)i * CM + J] = keval(P, sp, td[i], td[j]);
        }
    }
}

// pair -> (ta, tb), ta >= tb.  want_sigma: every pair of the lower triangle; else the ht tile columns
// of y' and the conditioning rows, then per pair of groups (ga >= gb) and date tile t the pair of
// their t-th tiles.
__device__ __forceinline__ bool lcomp_pair_of(const LongGeom &g, const LongCompGeom &cg, int pair,
                                              int &ta, int &tb) {
    const int nt = g.qpad / NB, ht = cg.hpad / NB, mt = cg.mpad / NB;
    if (g.want_sigma) {
        tri_decode(pair, ta, tb);
        return ta < nt;
    }
    if (pair < ht * nt) {
        tb = pair / nt;
        ta = pair % nt;
        return ta >= tb;
    }
    const int x = pair - ht * nt, t = x % mt;
    int ga, gb;
    tri_decode(x / mt, ga, gb);
    ta = ht + ga * mt + t;
    tb = ht + gb * mt + t;
    return ga < cg.cmax;
}

__global__ __launch_bounds__(256, 1) void lcomp_gram_kernel(LongGeom g, LongPtrs p, LongCompGeom cg,
                                                            LongCompPtrs cp, int npairs) {
    const int item = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pair = blockIdx.x * 4 + wave;
    if (pair >= npairs) return;
    int ta, tb;
    if (!lcomp_pair_of(g, cg, pair, ta, tb)) return;
    const int nc = lcomp_count(cp, item), ht = cg.hpad / NB, mt = cg.mpad / NB, m = cg.m;
    if (ta >= ht + nc * mt) return;                // a group the item does not have (tb <= ta)
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
    double *cr = cp.cross + (cp.cr_off[item] - cp.cr_off[0]) * m;
    const long CM = (long)nc * m;
    double *Sg = g.want_sigma ? cp.sigma + (cp.sig_off[item] - cp.sig_off[0]) : nullptr;
    // the tiles' groups and first dates are wave-uniform: -1 = y' and the conditioning rows
    const int ga = ta < ht ? -1 : (ta - ht) / mt, ia0 = ta < ht ? ta * NB : (ta - ht) % mt * NB;
    const int gb = tb < ht ? -1 : (tb - ht) / mt, ib0 = tb < ht ? tb * NB : (tb - ht) % mt * NB;
    const int n16 = lane & 15, isub = lane >> 4;
    const int jj0 = 4 * (n16 >> 2) + isub;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int it = 0; it < 4; ++it)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ia = ia0 + 16 * jt + jj0;                       // row of the A operand
                const int ib = ib0 + 16 * it + ((n16 + 4 * r) & 15);      // row of the B operand
                if (ia >= (ga < 0 ? cw : m) || ib >= (gb < 0 ? cw : m)) continue;
                if (ga == gb && ib > ia) continue;
                const double v = acc4[jt][it][r];
                if (gb < 0) {
                    const long ra = ga < 0 ? ia : cg.hpad + ga * cg.mpad + ia;
                    if (ib == 0) S[ra * cw] = v;
                    else S[ra * cw + ib] -= v;
                } else {
                    if (ia == ib) cr[((long)ga * nc + gb) * m + ia] -= v;
                    if (Sg) Sg[((long)ga * m + ia) * CM + (long)gb * m + ib] -= v;
                }
            }
}

// blockIdx.z = group.  The date's row of S_mc becomes its row of S_mc G^-T in place, as in
// long_apply_kernel; mu_g,s = (row . y') + (row of S_mc G^-T) . u_s.
__global__ __launch_bounds__(64) void lcomp_apply_kernel(LongGeom g, LongPtrs p, LongCompGeom cg,
                                                         LongCompPtrs cp) {
    const int item = blockIdx.y, grp = blockIdx.z;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= cg.m || grp >= lcomp_count(cp, item)) return;
    const int c = g.c, cw = c + 1, m = cg.m;
    const long r = cg.hpad + (long)grp * cg.mpad + i;
    double *mu = cp.mu + (long)(lcomp_first(cp, item) + grp) * g.D * m;
    if (p.info[item] > 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        for (int s = 0; s < g.D; ++s) mu[(long)s * m + i] = nan;
        return;
    }
    double *S = p.S + (long)item * g.q1 * cw;
    const double *Sc = S + cw + 1;
    double *w = S + r * cw + 1;
    for (int a = 0; a < c; ++a) {
        double s = w[a];
        for (int pp = 0; pp < a; ++pp) s -= w[pp] * Sc[a * cw + pp];
        w[a] = s / Sc[a * cw + a];
    }
    const double mu0 = g.n0 ? S[r * cw] : 0.0;
    for (int s = 0; s < g.D; ++s) {
        const double *z = p.z + ((long)item * g.D + s) * c;
        double x = mu0;
        for (int a = 0; a < c; ++a) x += w[a] * z[a];
        mu[(long)s * m + i] = x;
    }
}

// cross[ga][gb][i], ga >= gb, through long_schur_sub: the expression of sigma's entries, so cross is
// sigma's same-date diagonal bit for bit.  A thread owns both mirror images of its entry.
__global__ __launch_bounds__(64) void lcomp_cross_kernel(LongGeom g, LongPtrs p, LongCompGeom cg,
                                                         LongCompPtrs cp) {
    const int item = blockIdx.y;
    const int i = blockIdx.x * 64 + threadIdx.x;
    const int nc = lcomp_count(cp, item), m = cg.m;
    if (i >= m) return;
    const int c = g.c, cw = c + 1;
    const double *S = p.S + (long)item * g.q1 * cw;
    double *cr = cp.cross + (cp.cr_off[item] - cp.cr_off[0]) * m;
    const bool failed = p.info[item] > 0;
    for (int pr = blockIdx.z; pr < nc * (nc + 1) / 2; pr += gridDim.z) {
        int ga, gb;
        tri_decode(pr, ga, gb);
        double v;
        if (failed) {
            v = __longlong_as_double(0x7ff8000000000000LL);
        } else {
            const double *wa = S + (cg.hpad + (long)ga * cg.mpad + i) * cw + 1;
            const double *wb = S + (cg.hpad + (long)gb * cg.mpad + i) * cw + 1;
            v = long_schur_sub(cr[((long)ga * nc + gb) * m + i], wa, wb, c);
        }
        cr[((long)ga * nc + gb) * m + i] = v;
        cr[((long)gb * nc + ga) * m + i] = v;
    }
}

__global__ __launch_bounds__(256) void lcomp_sigma_kernel(LongGeom g, LongPtrs p, LongCompGeom cg,
                                                          LongCompPtrs cp) {
    const int item = blockIdx.y;
    const int c = g.c, cw = c + 1, m = cg.m;
    const long CM = (long)lcomp_count(cp, item) * m, total = CM * CM;
    double *Sg = cp.sigma + (cp.sig_off[item] - cp.sig_off[0]);
    const double *S = p.S + (long)item * g.q1 * cw;
    const bool failed = p.info[item] > 0;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long I = e / CM, J = e % CM;
        if (J > I) continue;
        double s;
        if (failed) {
            s = __longlong_as_double(0x7ff8000000000000LL);
        } else {
            const long ri = cg.hpad + I / m * cg.mpad + I % m, rj = cg.hpad + J / m * cg.mpad + J % m;
            s = long_schur_sub(Sg[I * CM + J], S + ri * cw + 1, S + rj * cw + 1, c);
        }
        Sg[I * CM + J] = s;
        Sg[J * CM + I] = s;
    }
}

}  // namespace ngp

// ngp_long_origin_kernels.h — ngp_factor_predict_origins: the forecasts of one resident factor from
// R forecast origins, origin r knowing the first cut[r] observations.
// Included from ngp_kernels.hip behind ngp_long_kernels.h, whose fill, small blocks, solve, products
// and conditioning block are used as they are (d = 0: the conditioning points are the tail).
//
// The leading c x c block of a Cholesky factor is the factor of the first c observations, so after
// long_solve_kernel every prefix of a panel row is a forecast origin: with v = row of the date and
// z = row 0,
//     mean_c = sum_{k < c} v_k z_k,     var_c = k(t*, t*) - sum_{k < c} v_k^2,
// and the same holds entry by entry through the conditioning block (the w of long_apply_kernel).
//
//   lorg_main_kernel   the origins inside the main block: ONE read of the solved date rows.  A wave
//                      owns 64 date rows; 64 x 64 tiles travel as full 512-byte rows into LDS
//                      (stride 65: the transposed read is conflict-free), lane j walks row j with k
//                      ascending and both running sums are stored whenever k reaches a cut.  Runs
//                      BEFORE long_gram_kernel: dg still holds the prior diagonal.
//   lorg_tail_kernel   one date per thread, the loop of long_apply_kernel, both sums stored whenever
//                      a reaches a cut behind the main block; NaN for an item that failed
//   lorg_logml_kernel  log p(y_1:c): the running -1/2 z_k^2 - log L_kk over the main block (the
//                      diagonal of L from the block inverses: L_kk = 1 / M_kk), on through G and u
//
// Every sum runs k ascending in one thread whatever the cuts of the call are, so an origin's bits
// depend neither on the other origins nor on the other items.
#pragma once
#include "ngp_internal.h"

namespace ngp {

constexpr int LORG_STRIDE = 65;        // doubles between the rows of a tile in LDS

// origin `cur` (the wave's cursor into the sorted cuts) of date i: the two running sums as they stand
__device__ __forceinline__ void lorg_emit(const LongGeom &g, const LongOriginGeom &og,
                                          const LongOriginPtrs &op, int item, int cur, int i,
                                          double sm, double sv, double kss, double nz) {
    if (i >= g.m) return;
    const long o = ((long)item * og.R + cur) * g.m + i;
    op.mu[o] = sm;
    op.var[o] = (kss - sv) + nz;
}

__global__ __launch_bounds__(64) void lorg_main_kernel(LongGeom g, LongPtrs p, LongOriginGeom og,
                                                       LongOriginPtrs op, DevSpec sp) {
    __shared__ double tile[64 * LORG_STRIDE];
    __shared__ double zt[64];
    const int item = blockIdx.y, lane = threadIdx.x;
    const int i = blockIdx.x * 64 + lane;                       // the lane's date
    const int row0 = g.c + 1 + blockIdx.x * 64;                 // panel row of lane 0
    const int rlast = g.q1 - 1;
    const long ld = g.ld;
    const double *W = p.W + (long)item * g.qpad * ld;
    const double kss = p.dg[(long)item * g.q1 + min(row0 + lane, rlast)];
    const double nz = g.noise_on_new ? p.progs[item].noise + sp.jitter : 0.0;
    const double *mine = tile + lane * LORG_STRIDE;
    double sm = 0.0, sv = 0.0;
    int cur = 0;
    int next = og.R0 > 0 ? op.cut[0] : 0x7fffffff;              // wave-uniform
    double nx[64], nz0;
#pragma unroll
    for (int r = 0; r < 64; ++r) nx[r] = W[(long)min(row0 + r, rlast) * ld + lane];
    nz0 = W[lane];
    for (int k0 = 0; k0 < g.n0 && cur < og.R0; k0 += 64) {
        __syncthreads();                                        // the walk of the tile before
#pragma unroll
        for (int r = 0; r < 64; ++r) tile[r * LORG_STRIDE + lane] = nx[r];
        zt[lane] = nz0;
        __syncthreads();
        if (k0 + 64 < g.n0) {                                   // the next tile, under the walk
#pragma unroll
            for (int r = 0; r < 64; ++r) nx[r] = W[(long)min(row0 + r, rlast) * ld + k0 + 64 + lane];
            nz0 = W[k0 + 64 + lane];
        }
        if (next > k0 + 64) {
#pragma unroll
            for (int k = 0; k < 64; ++k) {
                const double v = mine[k];
                sm = fma(v, zt[k], sm);
                sv = fma(v, v, sv);
            }
        } else {
            for (int k = 0; k < 64; ++k) {
                const double v = mine[k];
                sm = fma(v, zt[k], sm);
                sv = fma(v, v, sv);
                if (k0 + k + 1 == next) {
                    lorg_emit(g, og, op, item, cur, i, sm, sv, kss, nz);
                    ++cur;
                    next = cur < og.R0 ? op.cut[cur] : 0x7fffffff;
                }
            }
        }
    }
}

__global__ __launch_bounds__(64) void lorg_tail_kernel(LongGeom g, LongPtrs p, LongOriginGeom og,
                                                       LongOriginPtrs op, DevSpec sp) {
    const int item = blockIdx.y;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= g.m) return;
    const int c = g.c, cw = c + 1, r = c + 1 + i;
    double *mu = op.mu + (long)item * og.R * g.m + i;
    double *var = op.var + (long)item * og.R * g.m + i;
    if (p.info[item] > 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        for (int o = 0; o < og.R; ++o) {
            mu[(long)o * g.m] = nan;
            var[(long)o * g.m] = nan;
        }
        return;
    }
    if (og.R0 == og.R) return;
    double *S = p.S + (long)item * g.q1 * cw;
    const double *Sc = S + cw + 1;
    const double *z = p.z + (long)item * c;
    double *w = S + (long)r * cw + 1;             // the date's row of S_mc, then of W
    const double nz = g.noise_on_new ? p.progs[item].noise + sp.jitter : 0.0;
    double v = p.dg[(long)item * g.q1 + r];
    double x = g.n0 ? S[(long)r * cw] : 0.0;
    int cur = og.R0;
    int next = op.cut[cur] - g.n0;                // entries of the conditioning block the origin knows
    for (int a = 0; a < c && cur < og.R; ++a) {
        double s = w[a];
        for (int pp = 0; pp < a; ++pp) s -= w[pp] * Sc[a * cw + pp];
        const double wa = s / Sc[a * cw + a];
        w[a] = wa;
        v = fma(-wa, wa, v);
        x = fma(wa, z[a], x);
        if (a + 1 == next) {
            mu[(long)cur * g.m] = x;
            var[(long)cur * g.m] = v + nz;
            ++cur;
            next = cur < og.R ? op.cut[cur] - g.n0 : 0x7fffffff;
        }
    }
}

constexpr int LORG_TERMS = 1024;       // terms of the evidence formed side by side, then summed in order
__global__ __launch_bounds__(256) void lorg_logml_kernel(LongGeom g, LongPtrs p, LongOriginGeom og,
                                                         LongOriginPtrs op) {
    __shared__ double term[LORG_TERMS];
    const int item = blockIdx.x, tid = threadIdx.x;
    const double half_log_2pi = 0.91893853320467274178;
    double *out = op.logml + (long)item * og.R;
    if (p.info[item] > 0) {
        for (int o = tid; o < og.R; o += 256) out[o] = __longlong_as_double(0x7ff8000000000000LL);
        return;
    }
    double acc = 0.0;                             // thread 0's
    int cur = 0;
    const double *z0 = g.n0 ? p.W + (long)item * g.qpad * g.ld : nullptr;
    for (int k0 = 0; k0 < g.n0; k0 += LORG_TERMS) {
        const int cnt = min(LORG_TERMS, g.n0 - k0);
        __syncthreads();
        for (int e = tid; e < cnt; e += 256) {
            const int k = k0 + e, kk = k & (NB - 1);
            // M_j in strip order (chol_diag_kernel): element (kk, kk)
            const int strip = ((kk >> 2) << 2) | (kk >> 4);
            const int l = (kk & 3) | (((kk & 15) >> 2) << 2) | ((kk & 3) << 4);
            const double mkk = p.dinv[(long)(k / NB) * g.dinv_step + (long)item * (NB * NB) + strip * 64 + l];
            const double zk = z0[k];
            term[e] = fma(-0.5 * zk, zk, log(mkk));
        }
        __syncthreads();
        if (tid == 0)
            for (int e = 0; e < cnt; ++e) {
                acc += term[e];
                if (cur < og.R0 && k0 + e + 1 == op.cut[cur]) {
                    out[cur] = acc - (double)(k0 + e + 1) * half_log_2pi;
                    ++cur;
                }
            }
    }
    if (tid != 0) return;
    // on through the conditioning block: G and u of long_cond_kernel
    const int c = g.c, cw = c + 1;
    const double *Sc = p.S + (long)item * g.q1 * cw + cw + 1;
    const double *u = p.z + (long)item * c;
    for (int a = 0; a < c && cur < og.R; ++a) {
        acc += fma(-0.5 * u[a], u[a], -log(Sc[a * cw + a]));
        if (g.n0 + a + 1 == op.cut[cur]) {
            out[cur] = acc - (double)(g.n0 + a + 1) * half_log_2pi;
            ++cur;
        }
    }
}

}  // namespace ngp

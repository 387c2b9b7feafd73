// ngp_mixture_kernels.h — exact summaries of a Gaussian mixture's per-date marginals
// (ngp_mixture_cdf / ngp_mixture_quantiles / ngp_mixture_crps, include/ngp.h).
//
// The host stages a mixture DATE-MAJOR with its zero-weight components dropped: w [C], and per date
// j the rows mu [j][C], var [j][C] (ngp_host_mixture.h mixture_stage).  Everything here works on one date
// at a time and never looks at m, so a date's bits do not depend on which other dates travel with
// it.  All of it is fp64 VALU work bound by erf / exp / sqrt, not by memory: a date is 24 C bytes.
//
// Reductions are in a fixed order everywhere — a lane's strided partial, the wave by shuffles, the
// workgroup's waves through LDS in wave order, workgroups through a slab of partials that one
// workgroup per date sums — and nothing is accumulated with floating-point atomics: the same inputs
// give the same bits on every call.
//
//   mix_prep_kernel       inv = 1 / sqrt(2 var): the scale both the CDF and the density use
//   mix_cdf_kernel        one workgroup per (date, x): F(x) = sum_c w_c Phi((x - mu_c) / sd_c)
//   mix_quantile_kernel   one workgroup per (date, level) runs the WHOLE root search — bracket from
//                         the components, then Newton steps safeguarded by bisection, every step one
//                         CDF + density reduction of the workgroup; no launch per iteration, and a
//                         level's result cannot depend on the levels beside it
//   mix_crps_pairs_kernel the cross term  sum_(c < c') w_c w_c' A(mu_c - mu_c', var_c + var_c'):
//                         MIX_TILE x MIX_TILE tiles of the upper triangle, a thread keeps one row
//                         component in registers and walks the column tile in LDS; one partial per
//                         tile into the slab
//   mix_crps_final_kernel per date: E|X - y| and the diagonal of the cross term (w_c^2 2 sd_c /
//                         sqrt(pi)) over the components, the slab in tile order, CRPS out
//   mix_pair_rate_kernel  the pair expression on registers only (no loads, no LDS): what the fp64
//                         transcendental pipe gives at best, for ngp_microbench_mixture_pairs
#pragma once
#include "ngp_internal.h"

namespace ngp {

constexpr int MIX_THREADS = 256;      // every kernel here: four waves
constexpr int MIX_WAVES = MIX_THREADS / 64;
constexpr double MIX_INV_SQRT_PI = 0.56418958354775628695;   // 1 / sqrt(pi)
constexpr double MIX_BRACKET_SD = 40.0;    // Phi(-40) is zero in fp64: F(lo) = 0 < p for every p > 0
constexpr int MIX_MAX_ITERS = 400;

// total of v over the workgroup, the same value in every thread; sh holds MIX_WAVES doubles
__device__ __forceinline__ double mix_block_sum(double v, double *sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();            // sh may still be read from the previous reduction
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    double t = sh[0];
#pragma unroll
    for (int k = 1; k < MIX_WAVES; ++k) t += sh[k];
    return t;
}
__device__ __forceinline__ double mix_block_min(double v, double *sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_down(v, o, 64));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    double t = sh[0];
#pragma unroll
    for (int k = 1; k < MIX_WAVES; ++k) t = fmin(t, sh[k]);
    return t;
}

// A(d, v) = E|N(d, v)| = d erf(d / sqrt(2 v)) + sqrt(2 v / pi) exp(-d^2 / (2 v))
__device__ __forceinline__ double mix_abs_moment(double d, double v) {
    const double s = sqrt(2.0 * v);
    const double r = d / s;
    return d * erf(r) + s * MIX_INV_SQRT_PI * exp(-r * r);
}

__global__ __launch_bounds__(MIX_THREADS) void mix_prep_kernel(const double *var, double *inv,
                                                               int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * MIX_THREADS + threadIdx.x;
    if (i < n) inv[i] = 1.0 / sqrt(2.0 * var[i]);
}

// F and (optionally) the density at x for one date: every thread returns the workgroup's totals
template <bool DENSITY>
__device__ __forceinline__ void mix_cdf_at(int C, const double *__restrict__ w,
                                           const double *__restrict__ mu,
                                           const double *__restrict__ inv, double x, double *sh,
                                           double *F, double *f) {
    double aF = 0.0, af = 0.0;
    for (int c = threadIdx.x; c < C; c += MIX_THREADS) {
        const double wc = w[c], ic = inv[c];
        const double t = (x - mu[c]) * ic;
        aF += wc * (0.5 * erfc(-t));
        if (DENSITY) af += wc * ic * exp(-t * t);
    }
    *F = mix_block_sum(aF, sh);
    if (DENSITY) *f = mix_block_sum(af, sh) * MIX_INV_SQRT_PI;
}

// grid (K, m); x, out [m x K]
__global__ __launch_bounds__(MIX_THREADS) void mix_cdf_kernel(int C, int K, const double *w,
                                                              const double *mu, const double *inv,
                                                              const double *x, double *out) {
    __shared__ double sh[MIX_WAVES];
    const int k = blockIdx.x, j = blockIdx.y;
    double F, f;
    mix_cdf_at<false>(C, w, mu + (size_t)j * C, inv + (size_t)j * C, x[(size_t)j * K + k], sh, &F, &f);
    if (threadIdx.x == 0) out[(size_t)j * K + k] = F;
}

// grid (Q, m); q [m x Q].  Invariant of the search: F(lo) < p <= F(hi).  A Newton step from the
// last point is taken when it lands strictly inside the bracket, a bisection otherwise and on every
// fourth step (so the bracket halves at least that often whatever the shape of F).  It ends when
// the step no longer changes x or the bracket has no point left inside; every decision is taken
// from workgroup totals that all threads hold alike.
__global__ __launch_bounds__(MIX_THREADS) void mix_quantile_kernel(int C, int Q, const double *w,
                                                                   const double *mu,
                                                                   const double *inv,
                                                                   const double *probs, double *q) {
    __shared__ double sh[MIX_WAVES];
    const int k = blockIdx.x, j = blockIdx.y;
    const double *muj = mu + (size_t)j * C, *invj = inv + (size_t)j * C;
    const double p = probs[k];
    double lo = INFINITY, nhi = INFINITY;     // nhi: minus the upper end, so that one min serves both
    for (int c = threadIdx.x; c < C; c += MIX_THREADS) {
        const double r = MIX_BRACKET_SD * 0.70710678118654752440 / invj[c];   // 40 sd
        lo = fmin(lo, muj[c] - r);
        nhi = fmin(nhi, -(muj[c] + r));
    }
    lo = mix_block_min(lo, sh);
    double hi = -mix_block_min(nhi, sh);
    double x = 0.5 * lo + 0.5 * hi, res = hi;
    for (int it = 0; it < MIX_MAX_ITERS; ++it) {
        if (!(x > lo && x < hi)) { res = hi; break; }     // nothing left between lo and hi
        double F, f;
        mix_cdf_at<true>(C, w, muj, invj, x, sh, &F, &f);
        if (F < p) lo = x; else hi = x;
        res = hi;
        const double mid = 0.5 * lo + 0.5 * hi;
        double xn = mid;
        if ((it & 3) != 3 && f > 0.0) {
            const double xs = x - (F - p) / f;
            if (xs == x) { res = x; break; }              // the step no longer changes x
            if (xs > lo && xs < hi) xn = xs;
        }
        x = xn;
    }
    if (threadIdx.x == 0) q[(size_t)j * Q + k] = res;
}

static_assert(MIX_TILE == MIX_THREADS, "one row component per thread");

// grid (nt, nt, m), tiles with tj < ti leave at once; slab [m][nt (nt + 1) / 2] in (ti, tj >= ti) order
__global__ __launch_bounds__(MIX_THREADS) void mix_crps_pairs_kernel(int C, const double *w,
                                                                     const double *mu,
                                                                     const double *var,
                                                                     double *slab) {
    const int ti = blockIdx.x, tj = blockIdx.y, j = blockIdx.z, nt = gridDim.x;
    if (tj < ti) return;
    __shared__ double sw[MIX_TILE], sm[MIX_TILE], sv[MIX_TILE], sh[MIX_WAVES];
    const double *muj = mu + (size_t)j * C, *varj = var + (size_t)j * C;
    const int t = threadIdx.x;
    const int ci = ti * MIX_TILE + t, cj = tj * MIX_TILE + t;
    // padding beyond C: weight zero on a harmless component
    const double wi = ci < C ? w[ci] : 0.0, mi = ci < C ? muj[ci] : 0.0, vi = ci < C ? varj[ci] : 1.0;
    sw[t] = cj < C ? w[cj] : 0.0;
    sm[t] = cj < C ? muj[cj] : 0.0;
    sv[t] = cj < C ? varj[cj] : 1.0;
    __syncthreads();
    // a diagonal tile keeps the pairs above its diagonal: row component t meets columns t + 1 ...
    const int first = ti == tj ? t + 1 : 0;
    double acc = 0.0;
    for (int u = 0; u < MIX_TILE; ++u) {
        const double a = mix_abs_moment(mi - sm[u], vi + sv[u]);
        acc += (u >= first ? sw[u] : 0.0) * a;
    }
    const double tot = mix_block_sum(wi * acc, sh);
    if (t == 0)
        slab[(size_t)j * ((size_t)nt * (nt + 1) / 2) + (size_t)ti * nt - (size_t)ti * (ti - 1) / 2 +
             (tj - ti)] = tot;
}

// grid (m): crps[j] = T1 - (diag / 2 + pairs)
__global__ __launch_bounds__(MIX_THREADS) void mix_crps_final_kernel(int C, int64_t npairs,
                                                                     const double *w,
                                                                     const double *mu,
                                                                     const double *var,
                                                                     const double *y,
                                                                     const double *slab,
                                                                     double *crps) {
    __shared__ double sh[MIX_WAVES];
    const int j = blockIdx.x;
    const double *muj = mu + (size_t)j * C, *varj = var + (size_t)j * C;
    const double yj = y[j];
    double t1 = 0.0, dg = 0.0, pr = 0.0;
    for (int c = threadIdx.x; c < C; c += MIX_THREADS) {
        const double wc = w[c], vc = varj[c];
        t1 += wc * mix_abs_moment(yj - muj[c], vc);
        dg += wc * wc * (2.0 * MIX_INV_SQRT_PI * sqrt(vc));
    }
    for (int64_t k = threadIdx.x; k < npairs; k += MIX_THREADS) pr += slab[(size_t)j * npairs + k];
    t1 = mix_block_sum(t1, sh);
    dg = mix_block_sum(dg, sh);
    pr = mix_block_sum(pr, sh);
    if (threadIdx.x == 0) crps[j] = t1 - (0.5 * dg + pr);
}

// `iters` pair terms per thread on registers only; the operands drift so that nothing folds
__global__ __launch_bounds__(MIX_THREADS) void mix_pair_rate_kernel(int iters, double *out) {
    const double mi = 0.3 + 1e-3 * threadIdx.x, vi = 0.0025 + 1e-6 * blockIdx.x;
    double mj = 0.25, vj = 0.004, acc = 0.0;
    for (int u = 0; u < iters; ++u) {
        acc += 1e-4 * mix_abs_moment(mi - mj, vi + vj);
        mj += 1e-5;
        vj += 1e-8;
    }
    out[(size_t)blockIdx.x * MIX_THREADS + threadIdx.x] = acc;
}

void launch_mixture_prep(const double *var, double *inv, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(mix_prep_kernel, dim3((unsigned)((n + MIX_THREADS - 1) / MIX_THREADS)),
                       dim3(MIX_THREADS), 0, s, var, inv, n);
}
void launch_mixture_cdf(int C, int m, const double *w, const double *mu, const double *inv, int K,
                        const double *x, double *out, hipStream_t s) {
    hipLaunchKernelGGL(mix_cdf_kernel, dim3(K, m), dim3(MIX_THREADS), 0, s, C, K, w, mu, inv, x, out);
}
void launch_mixture_quantiles(int C, int m, const double *w, const double *mu, const double *inv,
                              int Q, const double *probs, double *q, hipStream_t s) {
    hipLaunchKernelGGL(mix_quantile_kernel, dim3(Q, m), dim3(MIX_THREADS), 0, s, C, Q, w, mu, inv,
                       probs, q);
}
void launch_mixture_crps(int C, int m, const double *w, const double *mu, const double *var,
                         const double *y, double *slab, double *crps, hipStream_t s) {
    const int nt = mix_tiles(C);
    hipLaunchKernelGGL(mix_crps_pairs_kernel, dim3(nt, nt, m), dim3(MIX_THREADS), 0, s, C, w, mu,
                       var, slab);
    hipLaunchKernelGGL(mix_crps_final_kernel, dim3(m), dim3(MIX_THREADS), 0, s, C,
                       mix_tile_pairs(C), w, mu, var, y, slab, crps);
}
void launch_mixture_pair_rate(int iters, int blocks, double *out, hipStream_t s) {
    hipLaunchKernelGGL(mix_pair_rate_kernel, dim3(blocks), dim3(MIX_THREADS), 0, s, iters, out);
}

}  // namespace ngp

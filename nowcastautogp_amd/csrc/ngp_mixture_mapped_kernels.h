// ngp_mixture_mapped_kernels.h — exact CRPS and mean of a Gaussian mixture's per-date marginals
// AFTER a monotone map psi = s o g (ngp_mixture_crps_mapped, include/ngp.h): g one of the inverse
// transformations of ngp_path_kernels.h (path_inv, edge rules included), s the score scale
// (identity, or log(. + shift)).  Included by ngp_kernels.hip after ngp_mixture_kernels.h (whose
// block reductions and 1 / sqrt(2 var) staging it uses) and ngp_path_kernels.h (path_inv).
//
// With Y = psi(X), yt = s(y), x0 the point where psi crosses yt (clipped to where psi moves):
//   CRPS(Y, yt) = int_{x < x0} F^2 dpsi + int_{x > x0} (1 - F)^2 dpsi + |yt - psi(x0)|
//   E[Y]        = psi(x0) + int_{x > x0} (1 - F) dpsi - int_{x < x0} F dpsi
// The last term of the CRPS is the stretch of the score axis between yt and the value psi takes at
// a clipped x0 (y beyond the range the forecast can reach); it vanishes when psi(x0) = yt.  Flat
// stretches of psi (clamp at 0, Box-Cox floor) contribute nothing and are not integrated: for every
// kind psi moves on ONE interval (xL, xR), so a date has at most two integration segments,
// [alo, x0] and [x0, ahi] with alo = max(lo, xL), ahi = min(hi, xR).
//
//   mixmap_scan_kernel    one workgroup per date: lo, hi, sd_min over the components (block
//                         minima: order-free), the boundaries of g, x0, psi(x0), the clip term and
//                         the date's flag into rec [m][MIXMAP_REC]
//   mixmap_panel_kernel   grid (tiles of 16 panels, work items): a thread owns ONE Gauss-Kronrod
//                         node of one panel; the components stream through LDS in tiles of
//                         MIX_TILE (w, mu, 1 / (sd sqrt 2)) and every node's sum_c w_c Phi runs in
//                         ascending c whatever the grid; the 15 nodes of a panel are folded by
//                         shuffles inside their 16 lanes; per panel K15 (CRPS), |K15 - G7|, K15
//                         (mean) into slab [work][maxp][3]
//   mixmap_reduce_kernel  one workgroup per work item: the panels in a fixed order (a thread's
//                         strided partial, the wave by shuffles, the waves in wave order)
// A work item is one date at one panel width (MixMapPlan, planned on the host from rec): the
// refinement loop relaunches only the dates whose error estimate is too large.  No kernel uses
// floating-point atomics and none looks at another date, so a date's bits depend on that date only.
#pragma once
#include "ngp_internal.h"

namespace ngp {

constexpr int MIXMAP_NODES = 15, MIXMAP_LANES = 16;           // lanes per panel (one idle)
constexpr int MIXMAP_PANELS_PER_WG = MIX_THREADS / MIXMAP_LANES;
static_assert(MIXMAP_PANELS_PER_WG == MIXMAP_TILE_PANELS, "the host sizes the grid by this");
// tail budget: a component's tail beyond k sd is cut where exp(-k^2 / 2 + L sd k) <= 1e-18, L the
// growth rate of psi' there (mixmap_growth): k = L sd + sqrt((L sd)^2 + K0^2), K0^2 = 2 ln 1e18
constexpr double MIXMAP_K0 = 9.1047490986831;
constexpr double MIXMAP_POLE_MASS = 1.0e-12;      // mass tolerated beyond a Box-Cox pole
constexpr double MIXMAP_BASE_FLOOR = 1.0e-10;     // the floor of path_inv's Box-Cox base

// Gauss-Kronrod 7/15 on [-1, 1]: abscissae 0..7 (outermost first, 7 = centre), Kronrod weights,
// Gauss weights of the odd abscissae
__constant__ double MIXMAP_XK[8] = {
    0.991455371120812639206854697526329, 0.949107912342758524526189684047851,
    0.864864423359769072789712788640926, 0.741531185599394439863864773280788,
    0.586087235467691130294144838258730, 0.405845151377397166906606412076961,
    0.207784955007898467600689403773245, 0.0};
__constant__ double MIXMAP_WK[8] = {
    0.022935322010529224963732008058970, 0.063092092629978553290700663189204,
    0.104790010322250183839876322541518, 0.140653259715525918745189590510238,
    0.169004726639267902826583426598550, 0.190350578064785409913256402421014,
    0.204432940075298892414161999234649, 0.209482141084727828012999174891714};
__constant__ double MIXMAP_WG[4] = {
    0.129484966168869693270611432679082, 0.279705391489276667901467771423780,
    0.381830050505118944950369775488975, 0.417959183673469387755102040816327};

struct MixMapArgs {
    ngp_inv_transform inv;
    int32_t scale;
    double shift;
};

__device__ __forceinline__ bool mixmap_is_exp(const ngp_inv_transform &t) {
    return t.kind == NGP_INV_EXP || (t.kind == NGP_INV_BOXCOX && t.lam == 0.0);
}

// s(v)
__device__ __forceinline__ double mixmap_score(const MixMapArgs &a, double v) {
    return a.scale == NGP_SCORE_LOG ? log(v + a.shift) : v;
}
__device__ __forceinline__ double mixmap_psi(const MixMapArgs &a, double x) {
    return mixmap_score(a, path_inv(a.inv, x));
}

// psi'(x) inside (xL, xR), where no edge rule of g is active
__device__ __forceinline__ double mixmap_dpsi(const MixMapArgs &a, double x) {
    const ngp_inv_transform &t = a.inv;
    double d = 1.0;
    if (mixmap_is_exp(t)) {
        d = exp(x);
    } else if (t.kind == NGP_INV_LOGISTIC100) {
        const double sg = 1.0 / (1.0 + exp(-x));
        d = 100.0 * sg * (1.0 - sg);
    } else if (t.kind == NGP_INV_BOXCOX) {
        d = pow(t.lam * x + 1.0, 1.0 / t.lam - 1.0);
    }
    if (a.scale == NGP_SCORE_LOG) d /= path_inv(t, x) + a.shift;
    return d;
}

// d ln psi' / dx towards the upper tail, from x on (0 where psi' does not grow)
__device__ __forceinline__ double mixmap_growth(const MixMapArgs &a, double x) {
    if (a.scale == NGP_SCORE_LOG) return 0.0;
    const ngp_inv_transform &t = a.inv;
    if (mixmap_is_exp(t)) return 1.0;
    if (t.kind == NGP_INV_BOXCOX) {
        const double base = t.lam * x + 1.0;
        if (!(base > 0.0) || t.lam >= 1.0) return 0.0;
        // lam < 0: the rate keeps rising towards the pole — twice the rate at x, see DESIGN 4.22
        return fmin((t.lam < 0.0 ? 2.0 : 1.0) * (1.0 - t.lam) / base, 64.0);
    }
    return 0.0;
}

// the interval (xL, xR) on which g moves, and g's value below xL
__device__ __forceinline__ void mixmap_bounds(const MixMapArgs &a, double *xL, double *xR,
                                              double *gmin) {
    const ngp_inv_transform &t = a.inv;
    double l = -INFINITY, r = INFINITY;
    if (t.kind == NGP_INV_IDENTITY) {
        *gmin = -INFINITY;
        if (a.scale == NGP_SCORE_LOG) l = -a.shift;          // log(x + shift) starts here
    } else {
        *gmin = path_inv(t, -INFINITY);
        if (mixmap_is_exp(t)) {
            if (t.offset > 0.0) l = log(t.offset);
        } else if (t.kind == NGP_INV_LOGISTIC100) {
            if (t.offset >= 100.0) l = INFINITY;
            else if (t.offset > 0.0) l = log(t.offset / (100.0 - t.offset));
        } else {
            if (t.lam > 0.0) l = (MIXMAP_BASE_FLOOR - 1.0) / t.lam;
            else r = (MIXMAP_BASE_FLOOR - 1.0) / t.lam;      // just below the pole
            if (t.offset > 0.0) l = fmax(l, (pow(t.offset, t.lam) - 1.0) / t.lam);
        }
    }
    *xL = l;
    *xR = r;
}

// inf { x : g(x) >= y }
__device__ __forceinline__ double mixmap_ginv(const MixMapArgs &a, double y, double gmin) {
    const ngp_inv_transform &t = a.inv;
    if (t.kind == NGP_INV_IDENTITY) return y;
    if (y <= gmin) return -INFINITY;
    const double v = y + t.offset;
    if (!(v > 0.0)) return -INFINITY;
    if (mixmap_is_exp(t)) return log(v);
    if (t.kind == NGP_INV_LOGISTIC100) {
        const double u = v / 100.0;
        return u >= 1.0 ? INFINITY : log(u / (1.0 - u));
    }
    return (pow(v, t.lam) - 1.0) / t.lam;
}

__device__ __forceinline__ double mixmap_block_max(double v, double *sh) {
    return -mix_block_min(-v, sh);
}

// grid (m); rec [m][MIXMAP_REC]
__global__ __launch_bounds__(MIX_THREADS) void mixmap_scan_kernel(int C, MixMapArgs a,
                                                                  const double *w, const double *mu,
                                                                  const double *inv, const double *y,
                                                                  double *rec) {
    __shared__ double sh[MIX_WAVES];
    const int j = blockIdx.x;
    const double *muj = mu + (size_t)j * C, *invj = inv + (size_t)j * C;
    double lo = INFINITY, hi0 = -INFINITY, sdmin = INFINITY;
    for (int c = threadIdx.x; c < C; c += MIX_THREADS) {
        const double sd = 0.70710678118654752440 / invj[c];
        lo = fmin(lo, muj[c] - MIXMAP_K0 * sd);
        hi0 = fmax(hi0, muj[c] + MIXMAP_K0 * sd);
        sdmin = fmin(sdmin, sd);
    }
    lo = mix_block_min(lo, sh);
    hi0 = mixmap_block_max(hi0, sh);
    sdmin = mix_block_min(sdmin, sh);
    const double L = mixmap_growth(a, hi0);
    double hi = hi0;
    if (L > 0.0) {
        hi = -INFINITY;
        for (int c = threadIdx.x; c < C; c += MIX_THREADS) {
            const double sd = 0.70710678118654752440 / invj[c];
            const double ls = L * sd;
            hi = fmax(hi, muj[c] + (ls + sqrt(ls * ls + MIXMAP_K0 * MIXMAP_K0)) * sd);
        }
        hi = mixmap_block_max(hi, sh);
    }
    double xL, xR, gmin;
    mixmap_bounds(a, &xL, &xR, &gmin);
    double flag = 0.0, beyond = 0.0;
    if (xR < hi) {       // Box-Cox, lam < 0: what lies beyond the pole maps to 0 — psi is not monotone
        double acc = 0.0;
        for (int c = threadIdx.x; c < C; c += MIX_THREADS)
            acc += w[c] * (0.5 * erfc((xR - muj[c]) * invj[c]));
        beyond = mix_block_sum(acc, sh);
        if (beyond > MIXMAP_POLE_MASS) flag = 3.0;
    }
    // the log of a value that is 0 (or below) where the forecast has mass: the score is infinite
    if (a.scale == NGP_SCORE_LOG && !(gmin + a.shift > 0.0) && xL > lo) flag = 3.0;
    const double alo = fmin(fmax(lo, xL), hi), ahi = fmax(fmin(hi, xR), alo);
    const double yj = y[j];
    const double xy = mixmap_ginv(a, yj, gmin);
    const double x0 = fmin(fmax(xy, alo), ahi);
    const double psi0 = mixmap_psi(a, x0), yt = mixmap_score(a, yj);
    const double clip = (xy > alo && xy < ahi) ? 0.0 : fabs(yt - psi0);
    if (threadIdx.x == 0) {
        double *r = rec + (size_t)j * MIXMAP_REC;
        r[MIXMAP_REC_LO] = lo;
        r[MIXMAP_REC_HI] = hi;
        r[MIXMAP_REC_SDMIN] = sdmin;
        r[MIXMAP_REC_ALO] = alo;
        r[MIXMAP_REC_AHI] = ahi;
        r[MIXMAP_REC_X0] = x0;
        r[MIXMAP_REC_PSI0] = psi0;
        r[MIXMAP_REC_CLIP] = clip;
        r[MIXMAP_REC_FLAG] = flag;
        r[MIXMAP_REC_BEYOND] = beyond;
    }
}

// grid (tiles, work); slab [work][maxp][3]
__global__ __launch_bounds__(MIX_THREADS) void mixmap_panel_kernel(int C, MixMapArgs a, int maxp,
                                                                   const MixMapPlan *plans,
                                                                   const double *w, const double *mu,
                                                                   const double *inv, double *slab) {
    const MixMapPlan pl = plans[blockIdx.y];
    const int first = blockIdx.x * MIXMAP_PANELS_PER_WG;
    if (first >= pl.npanels) return;                       // the whole workgroup alike
    __shared__ double sw[MIX_TILE], sm[MIX_TILE], si[MIX_TILE];
    const int t = threadIdx.x;
    const int p = first + (t >> 4), n = t & (MIXMAP_LANES - 1);
    const bool live = p < pl.npanels && n < MIXMAP_NODES;
    // segment 0, [alo, x0]: the integrand is built on F; segment 1, [x0, ahi]: on 1 - F
    const bool upper = p >= pl.n0;
    const double h = upper ? pl.h1 : pl.h0;
    const double left = upper ? pl.a1 + (double)(p - pl.n0) * h : pl.a0 + (double)p * h;
    const int i = n < 8 ? n : 14 - n;                      // abscissa; n = 15 (idle) gives -1
    const int ia = live ? i : 7;
    const double x = left + 0.5 * h + 0.5 * h * (n < 7 ? -MIXMAP_XK[ia] : MIXMAP_XK[ia]);
    const double sgn = upper ? 1.0 : -1.0;
    const double *muj = mu + (size_t)pl.date * C, *invj = inv + (size_t)pl.date * C;
    double T = 0.0;
    for (int c0 = 0; c0 < C; c0 += MIX_TILE) {
        const int c = c0 + t;
        __syncthreads();                                   // the previous tile is done with
        sw[t] = c < C ? w[c] : 0.0;                        // padding: weight zero on a harmless one
        sm[t] = c < C ? muj[c] : 0.0;
        si[t] = c < C ? invj[c] : 1.0;
        __syncthreads();
        const int nu = min(MIX_TILE, C - c0);
        for (int u = 0; u < nu; ++u) T += sw[u] * (0.5 * erfc(sgn * ((x - sm[u]) * si[u])));
    }
    double kc = 0.0, gc = 0.0, km = 0.0;
    if (live) {
        const double d = mixmap_dpsi(a, x) * (0.5 * h);
        kc = MIXMAP_WK[ia] * (T * T * d);
        km = MIXMAP_WK[ia] * (T * d);
        if (ia & 1) gc = MIXMAP_WG[ia >> 1] * (T * T * d);
    }
#pragma unroll
    for (int o = MIXMAP_LANES / 2; o > 0; o >>= 1) {
        kc += __shfl_down(kc, o, MIXMAP_LANES);
        gc += __shfl_down(gc, o, MIXMAP_LANES);
        km += __shfl_down(km, o, MIXMAP_LANES);
    }
    if (n == 0 && p < pl.npanels) {
        double *out = slab + ((size_t)blockIdx.y * maxp + p) * 3;
        out[0] = kc;
        out[1] = fabs(kc - gc);
        out[2] = upper ? km : -km;
    }
}

// grid (work); res [work][3]: the two integrals and the error estimate, panels in a fixed order
__global__ __launch_bounds__(MIX_THREADS) void mixmap_reduce_kernel(int maxp, const MixMapPlan *plans,
                                                                    const double *slab, double *res) {
    __shared__ double sh[MIX_WAVES];
    const int np = plans[blockIdx.x].npanels;
    const double *s = slab + (size_t)blockIdx.x * maxp * 3;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int p = threadIdx.x; p < np; p += MIX_THREADS) {
        a0 += s[(size_t)p * 3];
        a1 += s[(size_t)p * 3 + 1];
        a2 += s[(size_t)p * 3 + 2];
    }
    a0 = mix_block_sum(a0, sh);
    a1 = mix_block_sum(a1, sh);
    a2 = mix_block_sum(a2, sh);
    if (threadIdx.x == 0) {
        res[(size_t)blockIdx.x * 3] = a0;
        res[(size_t)blockIdx.x * 3 + 1] = a1;
        res[(size_t)blockIdx.x * 3 + 2] = a2;
    }
}

void launch_mixmap_scan(int C, int m, const ngp_inv_transform &inv, int scale, double shift,
                        const double *w, const double *mu, const double *invsd, const double *y,
                        double *rec, hipStream_t s) {
    const MixMapArgs a{inv, scale, shift};
    hipLaunchKernelGGL(mixmap_scan_kernel, dim3(m), dim3(MIX_THREADS), 0, s, C, a, w, mu, invsd, y,
                       rec);
}
void launch_mixmap_panels(int C, int nwork, int maxp, const ngp_inv_transform &inv, int scale,
                          double shift, const MixMapPlan *plans, const double *w, const double *mu,
                          const double *invsd, double *slab, double *res, hipStream_t s) {
    const MixMapArgs a{inv, scale, shift};
    const int tiles = (maxp + MIXMAP_PANELS_PER_WG - 1) / MIXMAP_PANELS_PER_WG;
    if (tiles > 0)
        hipLaunchKernelGGL(mixmap_panel_kernel, dim3(tiles, nwork), dim3(MIX_THREADS), 0, s, C, a,
                           maxp, plans, w, mu, invsd, slab);
    hipLaunchKernelGGL(mixmap_reduce_kernel, dim3(nwork), dim3(MIX_THREADS), 0, s, maxp, plans, slab,
                       res);
}

}  // namespace ngp

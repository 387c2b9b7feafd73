// ngp_long_sample_indep_kernels.h — ngp_factor_sample_long_indep: the pick and the normals of S
// independent mixtures over the items of ONE long query.  Included from
// ngp_kernels.hip behind ngp_long_sample_kernels.h, whose count, grouping, padding, factorisation
// and product it uses as they are: items s P' .. (s + 1) P' - 1 are the components of mixture s,
// path (s, d) is keyed by seeds[s] with scenario counter 0 — the path ngp_factor_sample_long draws
// for (seed = seeds[s], S = 1) on a factor of that mixture's items alone.
//
//   lsi_pick_kernel     one thread per (mixture, draw): the item (for the grouping) and the
//                       component within the mixture (for the caller)
//   lsi_normals_kernel  z of the staged paths, once per path: Z [sorted position][mpad]
#pragma once
#include "ngp_internal.h"

namespace ngp {

__global__ __launch_bounds__(LS_THREADS) void lsi_pick_kernel(LongSampleGeom g, int Pm, const double *w,
                                                              const uint64_t *seeds, int32_t *item,
                                                              int32_t *comp) {
    const long idx = (long)blockIdx.x * LS_THREADS + threadIdx.x;
    if (idx >= g.N) return;
    const int s = (int)(idx / g.draws), d = (int)(idx % g.draws);
    const uint64_t seed = seeds[s];
    // block 0 of the mixture's own stream: inverse CDF over its own P' weights
    const Philox4 r0 = philox4x32_10(Philox4{(unsigned)d, 0u, 0u, 0u}, (unsigned)seed, (unsigned)(seed >> 32));
    const double u = u01(r0.x, r0.y);
    const double *ws = w + (long)s * Pm;
    int k = Pm - 1;
    double acc = 0.0;
    for (int i = 0; i < Pm; ++i) {
        acc += ws[i];
        if (u < acc) { k = i; break; }
    }
    item[idx] = s * Pm + k;
    comp[idx] = k;
}

// Z [row][mpad], row r the path at sorted position zfirst + r, keyed by the seed of its own
// mixture: blocks 1 + j / 2, one Box-Muller pair per thread, a row written in full (the second
// normal of the last pair of an odd m and the padding are 0)
__global__ __launch_bounds__(LS_THREADS) void lsi_normals_kernel(LongSampleGeom g, const uint64_t *seeds,
                                                                 const int32_t *order, long zfirst,
                                                                 long zrows, double *Z) {
    const int half = g.mpad / 2;
    const long e = (long)blockIdx.x * LS_THREADS + threadIdx.x;
    if (e >= zrows * half) return;
    const long r = e / half;
    const int j0 = 2 * (int)(e % half);
    double z0 = 0.0, z1 = 0.0;
    if (j0 < g.m) {
        const long idx = order[zfirst + r];
        const int s = (int)(idx / g.draws), d = (int)(idx % g.draws);
        const uint64_t seed = seeds[s];
        const Philox4 q = philox4x32_10(Philox4{(unsigned)d, 0u, (unsigned)(1 + j0 / 2), 0u}, (unsigned)seed,
                                        (unsigned)(seed >> 32));
        const double u1 = u01(q.x, q.y), u2 = u01(q.z, q.w);
        const double rad = sqrt(-2.0 * log(u1)), ang = 2.0 * M_PI * u2;
        z0 = rad * cos(ang);
        if (j0 + 1 < g.m) z1 = rad * sin(ang);
    }
    f64x2 v;
    v.x = z0;
    v.y = z1;
    *reinterpret_cast<f64x2 *>(Z + r * g.mpad + j0) = v;
}

void launch_lsi_pick(const LongSampleGeom &g, int Pm, const double *w, const uint64_t *seeds, int32_t *item,
                     int32_t *comp, hipStream_t s) {
    hipLaunchKernelGGL(lsi_pick_kernel, dim3((unsigned)((g.N + LS_THREADS - 1) / LS_THREADS)), dim3(LS_THREADS),
                       0, s, g, Pm, w, seeds, item, comp);
}
void launch_lsi_normals(const LongSampleGeom &g, const uint64_t *seeds, const int32_t *order, int64_t zfirst,
                        int64_t zrows, double *Z, hipStream_t s) {
    const int64_t n = zrows * (g.mpad / 2);
    hipLaunchKernelGGL(lsi_normals_kernel, dim3((unsigned)((n + LS_THREADS - 1) / LS_THREADS)), dim3(LS_THREADS),
                       0, s, g, seeds, order, (long)zfirst, (long)zrows, Z);
}

}  // namespace ngp

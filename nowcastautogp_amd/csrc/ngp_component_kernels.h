// ngp_component_kernels.h — the additive decomposition of a resident factor's forecast
// (ngp_factor_components; conditioned on appended points and scenarios:
// ngp_factor_components_nowcast, section 4.20).  Included from ngp_kernels.hip behind
// ngp_tree_kernels.h: the interpreter (keval, keval_reduced) is the one of the fills.
//
// The query is a plain factor query whose m' = Cmax m forecast rows are regrouped: row (c, j) of an
// item is date j under the item's c-th component program instead of the item's own.  The sweep and
// the Gram kernel see aux rows like any other; what knows about components is
//   component_fill_kernel      the component rows against the main-block columns
//   component_epilogue_kernel  the elimination of the tail and the appended points with k_c in the
//                              cross terms and the block-diagonal prior, the per-scenario solves,
//                              mu / sigma / var in the caller's packed layout
// The tail rows, the appended rows and the y' row stay with the aux fill under the item's own program.
#pragma once
#include "ngp_internal.h"
#include "ngp_tree_kernels.h"

namespace ngp {

// One workgroup = (64-column block, 64 dates) of ONE component of one item: the program in LDS is
// uniform over the workgroup, so the interpreter never diverges.  Thread = (column pair, row group)
// as in the fills: 16-byte stores.  Components an item does not have (c >= C_p) are zero rows.
__global__ __launch_bounds__(256) void component_fill_kernel(JobGeom g, ChunkPtrs p, CompPtrs cp,
                                                             DevSpec sp) {
    __shared__ DevProgram P;
    const int item = blockIdx.y, c = blockIdx.z;
    const int c0 = cp.first[item];
    const bool live = c < cp.first[item + 1] - c0;
    if (live) load_program(&P, cp.progs + c0 + c);
    __syncthreads();
    const int bc = blockIdx.x % g.nb0, jt = blockIdx.x / g.nb0;
    const int ty = threadIdx.x >> 5;
    const int col = bc * NB + 2 * (threadIdx.x & 31);
    double *Lit = p.L + (long)item * g.item_stride;
    const double t2a = p.t0[col], t2b = p.t0[col + 1];
    const int jend = min(cp.m, jt * NB + NB);
    for (int j = jt * NB + ty; j < jend; j += 8) {
        const int ar = g.da + c * cp.m + j;       // aux row: behind the tail, component-major
        f64x2 v = {0.0, 0.0};
        if (live) {
            const double t1 = p.taux[ar];
            v.x = keval(P, sp, t1, t2a);
            v.y = keval(P, sp, t1, t2b);
        }
        *reinterpret_cast<f64x2 *>(Lit + ((long)g.n0 + ar) * g.ld + col) = v;
    }
}

// Schur-complement algebra of the component rows on G (one single-wave workgroup per item), the
// epilogue's with k_c in the cross terms (ngp_factor_components: d = 0 and one scenario;
// ngp_factor_components_nowcast: d appended points, D scenarios — ONE code path):
//   A = tail rows then appended points (da), (c, j) = component rows, Y = data row
//   S_AA = K_AA + nz I - G_AA = L_A L_A'  under k   z_A,s = L_A^-1 (y_A,s - G_AY)  per scenario
//   V_c  = (k_c(t*, t_A) - G_cA) L_A^-T            mu_c,s = G_cY + V_c z_A,s
//   Sigma_cc' = delta_cc' k_c(t*, t*) - G_cc' - V_c V_c'     (the same for every scenario)
//   logml_full[s] = -1/2 (G_YY + |z_A,s|^2) - (logdet0 + sum log diag L_A) - (n + d)/2 log 2pi
// L_A, the solve vector, log diag L_A and the right-hand side live in dynamic LDS while
// (da^2 + 4 da) doubles fit COMP_EPI_LDS_BYTES (da <= 76; lds_work != 0), else behind V in the
// per-item work buffer, as epilogue_kernel switches; V and the prior's diagonal are always in the
// work buffer.  Every sum runs in a fixed order and every scenario goes through the same wave-wide
// solve, one after the other: a scenario's bits depend neither on D nor on its place.  sigma and
// var come from ONE loop (an entry of the diagonal is the same expression either way), so var is
// the diagonal of sigma bit for bit whether or not sigma is asked for.
__global__ __launch_bounds__(64) void component_epilogue_kernel(JobGeom g, EpiPtrs p, CompPtrs cp,
                                                                DevSpec sp, int lds_work) {
    __shared__ DevProgram P;     // the item's own program: A x A
    __shared__ DevProgram Pc;    // one component at a time
    __shared__ int bad;
    extern __shared__ double comp_dyn[];
    const int item = blockIdx.x, tid = threadIdx.x;
    load_program(&P, p.progs + item);
    if (tid == 0) bad = 0;
    __syncthreads();
    const int da = g.da, na = g.naux, Y = da + g.m, m = cp.m, D = g.D;
    const int c0 = cp.first[item], nc = cp.first[item + 1] - c0, CM = nc * m;
    const double nz = P.noise + sp.jitter;
    const double *G = p.G + (long)item * na * na;
    const double *tab = p.tab ? p.tab + (long)item * g.maxstat * g.R : nullptr;
    const double *sig = p.sig ? p.sig + (long)item * g.maxcp * g.npts : nullptr;
    auto kaux = [&](int u, int v) -> double {   // the item's kernel between two points of A
        if (tab)
            return keval_reduced(P, tab, sig, g.R, g.npts, p.taux[u], p.taux[v],
                                 abs(p.qpts[g.n0 + u] - p.qpts[g.n0 + v]), g.n0 + u, g.n0 + v);
        return keval(P, sp, p.taux[u], p.taux[v]);
    };
    double *VA = p.work + (long)item * p.work_stride;    // [CM x da]
    double *pd = VA + (long)cp.cmax * m * da;            // [CM] prior variances
    double *LA = lds_work ? comp_dyn : pd + (long)cp.cmax * m;   // [da x da]
    double *z = LA + (long)da * da;                      // [da] the scenario's solve vector
    double *ldA = z + da;                                // [da] log diag L_A
    double *rhs = ldA + da;                              // [da] the scenario's y_A - G_AY
    double *mu = cp.mu + (long)c0 * D * m;               // [nc][D][m]
    double *var = cp.var ? cp.var + (long)c0 * m : nullptr;
    double *Sg = cp.sigma ? cp.sigma + cp.sig_off[item] : nullptr;
    const int info0 = p.info[item];

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
    for (int k = 0; k < da; ++k) {  // in-place right-looking Cholesky of S_AA, as the epilogue's
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
    // component by component (the program in LDS is the wave's): cross terms against A and the
    // prior block — the lower triangle into sigma when it is asked for, else the diagonal alone
    for (int c = 0; c < nc; ++c) {
        __syncthreads();
        load_program(&Pc, cp.progs + c0 + c);
        __syncthreads();
        const double *ts = p.taux + da + c * m;
        for (int e = tid; e < m * da; e += 64) {
            const int j = e / da, a = e % da;
            VA[(long)(c * m + j) * da + a] =
                keval(Pc, sp, ts[j], p.taux[a]) - (g.n0 ? G[(da + c * m + j) * na + a] : 0.0);
        }
        const int cnt = Sg ? m * m : m;
        for (int e = tid; e < cnt; e += 64) {
            const int j = Sg ? e / m : e, j2 = Sg ? e % m : e;
            if (j2 > j) continue;
            const double v = keval(Pc, sp, ts[j], ts[j2]);
            if (Sg) Sg[(long)(c * m + j) * CM + c * m + j2] = v;
            if (j == j2) pd[c * m + j] = v;
        }
    }
    __syncthreads();
    // V: one component row per thread, forward substitution along A
    for (int i = tid; i < CM; i += 64) {
        double *Vi = VA + (long)i * da;
        for (int a = 0; a < da; ++a) {
            double s = Vi[a];
            for (int pp = 0; pp < a; ++pp) s -= Vi[pp] * LA[a * da + pp];
            Vi[a] = s / LA[a * da + a];
        }
    }
    __syncthreads();
    // scenario by scenario: z_A (every row's dot product spread over the lanes), the evidence, the
    // components' means
    const double q0 = g.n0 ? G[Y * na + Y] : 0.0;
    const double ld0 = p.logdet[item];
    const double LOG2PI = 1.8378770664093454836;
    const double *ya_base = p.ya + (g.y_shared ? 0 : (long)item * D * da);
    for (int s = 0; s < D; ++s) {
        const double *ya = ya_base + (long)s * da;
        for (int a = tid; a < da; a += 64) rhs[a] = ya[a] - (g.n0 ? G[a * na + Y] : 0.0);
        __syncthreads();
        double quad = 0.0, ldsum = 0.0;
        for (int a = 0; a < da; ++a) {
            double part = 0.0;
            for (int pp = tid; pp < a; pp += 64) part += LA[a * da + pp] * z[pp];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
            const double e = (rhs[a] - part) / LA[a * da + a];
            if (tid == 0) z[a] = e;
            __syncthreads();
            quad += e * e;
            ldsum += ldA[a];
        }
        if (tid == 0 && p.logml_full)
            p.logml_full[(long)item * D + s] =
                -0.5 * (q0 + quad) - (ld0 + ldsum) - 0.5 * (g.n0 + da) * LOG2PI;
        for (int i = tid; i < CM; i += 64) {
            const double *Vi = VA + (long)i * da;
            double v = g.n0 ? G[(da + i) * na + Y] : 0.0;
            for (int a = 0; a < da; ++a) v += Vi[a] * z[a];
            mu[((long)(i / m) * D + s) * m + i % m] = v;
        }
        __syncthreads();
    }
    {
        const int cnt = Sg ? CM * CM : CM;
        for (int e = tid; e < cnt; e += 64) {
            const int i = Sg ? e / CM : e, i2 = Sg ? e % CM : e;
            if (i2 > i) continue;
            double s = 0.0;
            if (i / m == i2 / m) s = (i == i2) ? pd[i] : Sg[(long)i * CM + i2];
            s -= g.n0 ? G[(da + i) * na + da + i2] : 0.0;
            const double *Vi = VA + (long)i * da, *Vj = VA + (long)i2 * da;
            for (int a = 0; a < da; ++a) s -= Vi[a] * Vj[a];
            if (Sg) {
                Sg[(long)i * CM + i2] = s;
                Sg[(long)i2 * CM + i] = s;
            }
            if (i == i2 && var) var[i] = s;
        }
    }
    __syncthreads();
    // a failed item (its factor at creation, or a pivot of A here): NaN in every output
    if (info0 > 0 || bad) {
        for (int i = tid; i < CM * D; i += 64) mu[i] = NAN;
        if (var)
            for (int i = tid; i < CM; i += 64) var[i] = NAN;
        if (Sg)
            for (int e = tid; e < CM * CM; e += 64) Sg[e] = NAN;
        if (p.logml_full)
            for (int s = tid; s < D; s += 64) p.logml_full[(long)item * D + s] = NAN;
    }
    if (tid == 0 && bad && info0 <= 0) p.info[item] = g.n0 + bad;
}

}  // namespace ngp

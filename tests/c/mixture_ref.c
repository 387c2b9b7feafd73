/* mixture_ref.c — extended-precision reference for the summaries of a Gaussian mixture's per-date
 * marginals (include/ngp.h: ngp_mixture_cdf / ngp_mixture_quantiles / ngp_mixture_crps).
 *
 * The four formulas of the header in long double (erfl, erfcl, expl, sqrtl), plain loops in the
 * order the components come, and a bisection on the long-double CDF for the quantiles.  Built as a
 * shared object by tests/mixture_reference.py with the system C compiler; nothing of the library
 * is used here.  Dates are independent, so the loop over dates may run in parallel (-fopenmp): a
 * date's sums stay serial.
 *
 * Layout as in the header: w [C], mu [C x m], var [C x m]; components of weight zero are skipped.
 */
#include <math.h>
#include <stdint.h>

#define SQRT2L 1.41421356237309504880168872420969808L
#define PIL 3.14159265358979323846264338327950288L

static long double cdf_one(int C, int m, const double *w, const double *mu, const double *var, int j,
                           long double x, long double *dens) {
    long double F = 0.0L, f = 0.0L;
    for (int c = 0; c < C; ++c) {
        if (!(w[c] > 0.0)) continue;
        const long double sd = sqrtl((long double)var[(int64_t)c * m + j]);
        const long double z = (x - (long double)mu[(int64_t)c * m + j]) / sd;
        F += (long double)w[c] * 0.5L * erfcl(-z / SQRT2L);
        f += (long double)w[c] * expl(-0.5L * z * z) / (sd * sqrtl(2.0L * PIL));
    }
    if (dens) *dens = f;
    return F;
}

/* E|N(d, v)| */
static long double abs_moment(long double d, long double v) {
    return d * erfl(d / sqrtl(2.0L * v)) + sqrtl(2.0L * v / PIL) * expl(-d * d / (2.0L * v));
}

/* F [m x K] and the density [m x K] at x [m x K]; minus_p != NULL: F - p[k] in long double before
 * the rounding to double (what a quantile is judged by) */
void mixref_cdf(int C, int m, const double *w, const double *mu, const double *var, int K,
                const double *x, const double *minus_p, double *F, double *dens) {
#pragma omp parallel for schedule(dynamic, 1)
    for (int j = 0; j < m; ++j)
        for (int k = 0; k < K; ++k) {
            long double f;
            long double v = cdf_one(C, m, w, mu, var, j, (long double)x[(int64_t)j * K + k], &f);
            if (minus_p) v -= (long double)minus_p[k];
            F[(int64_t)j * K + k] = (double)v;
            dens[(int64_t)j * K + k] = (double)f;
        }
}

/* q [m x Q]: bisection from mean -+ 40 sd of the components to a bracket of 1e-18 relative width */
void mixref_quantiles(int C, int m, const double *w, const double *mu, const double *var, int Q,
                      const double *probs, double *q) {
#pragma omp parallel for schedule(dynamic, 1)
    for (int j = 0; j < m; ++j) {
        long double lo0 = INFINITY, hi0 = -INFINITY;
        for (int c = 0; c < C; ++c) {
            if (!(w[c] > 0.0)) continue;
            const long double sd = sqrtl((long double)var[(int64_t)c * m + j]);
            const long double mc = (long double)mu[(int64_t)c * m + j];
            if (mc - 40.0L * sd < lo0) lo0 = mc - 40.0L * sd;
            if (mc + 40.0L * sd > hi0) hi0 = mc + 40.0L * sd;
        }
        for (int k = 0; k < Q; ++k) {
            long double lo = lo0, hi = hi0;
            const long double p = (long double)probs[k];
            for (int it = 0; it < 400; ++it) {
                const long double mid = 0.5L * lo + 0.5L * hi;
                if (!(mid > lo && mid < hi)) break;
                if (cdf_one(C, m, w, mu, var, j, mid, 0) < p) lo = mid; else hi = mid;
                if (hi - lo <= 1e-18L * fmaxl(fabsl(lo), fabsl(hi))) break;
            }
            q[(int64_t)j * Q + k] = (double)(0.5L * lo + 0.5L * hi);
        }
    }
}

/* For ny observation vectors y [ny x m]: crps [ny x m], t1 [ny x m] = sum_c w_c A(y - mu_c, var_c),
 * and t2 [m] = sum_c sum_c' w_c w_c' A(mu_c - mu_c', var_c + var_c') (it does not depend on y);
 * only_date >= 0: that date alone (the others are left untouched) */
void mixref_crps(int C, int m, const double *w, const double *mu, const double *var, int ny,
                 const double *y, int only_date, double *crps, double *t1, double *t2) {
#pragma omp parallel for schedule(dynamic, 1)
    for (int j = 0; j < m; ++j) {
        if (only_date >= 0 && j != only_date) continue;
        long double a2 = 0.0L;
        for (int c = 0; c < C; ++c) {
            if (!(w[c] > 0.0)) continue;
            const long double mc = (long double)mu[(int64_t)c * m + j];
            const long double vc = (long double)var[(int64_t)c * m + j];
            long double row = 0.0L;       /* pairs c' > c count twice, the diagonal once */
            for (int e = c + 1; e < C; ++e) {
                if (!(w[e] > 0.0)) continue;
                row += (long double)w[e] * abs_moment(mc - (long double)mu[(int64_t)e * m + j],
                                                      vc + (long double)var[(int64_t)e * m + j]);
            }
            a2 += (long double)w[c] * (2.0L * row + (long double)w[c] * abs_moment(0.0L, 2.0L * vc));
        }
        t2[j] = (double)a2;
        for (int r = 0; r < ny; ++r) {
            long double a1 = 0.0L;
            for (int c = 0; c < C; ++c) {
                if (!(w[c] > 0.0)) continue;
                a1 += (long double)w[c] * abs_moment((long double)y[(int64_t)r * m + j] -
                                                         (long double)mu[(int64_t)c * m + j],
                                                     (long double)var[(int64_t)c * m + j]);
            }
            crps[(int64_t)r * m + j] = (double)(a1 - 0.5L * a2);
            t1[(int64_t)r * m + j] = (double)a1;
        }
    }
}

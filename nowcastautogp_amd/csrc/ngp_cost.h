// ngp_cost.h — the roofline accounting of the launches: timing class (include/ngp.h), algorithmic
// flops and HBM bytes of each launch the schedule issues, as pure functions of the geometry.
// ngp_profile is a public output (bench.py derives the roofline fractions of the README from it);
// tests/golden/route_trace_v1.txt holds these numbers to the last digit.
#pragma once

namespace ngp {

struct Cost { int cls; double flops, bytes; };

// chol_small_kernel: factor + the aux rows' solves and updates of the whole item in one launch
inline double small_flops(const JobGeom &g, const SmallPlan &pl) {
    const double n = 16.0 * pl.nbe;
    double f = n * n * n / 3.0;
    if (pl.ident) f += n * n * n / 3.0 + n * n;
    else f += (double)g.naux * n * n;
    return f;
}
inline Cost cost_small(const JobGeom &g, const SmallPlan &pl, int bc) {
    const double nn = 16.0 * pl.nbe;
    return {13, bc * small_flops(g, pl), bc * 8.0 * (nn * nn * (pl.ident ? 1.5 : 1.0) + 2.0 * g.naux * nn)};
}
// diag_ahead_kernel of tile (jj + 2, jj + 2) at step jj (class 8: on the side stream)
inline Cost cost_ahead(int bc, int jj) {
    const double k = (double)jj * NB;
    return {8, bc * (double)NB * NB * k, bc * 8.0 * NB * k};
}
inline Cost cost_diag(int bc, int jj, int k0_diag) {
    const double kd = (double)jj * NB - k0_diag;
    return {1, bc * ((double)NB * NB * kd + (double)NB * NB * NB / 3.0), bc * 8.0 * (NB * kd + 2.0 * NB * NB)};
}
// Toeplitz jobs: the share of a chunk's items whose main tiles are regenerated, not read
inline double lazy_fraction(const JobGeom &g, int n_fill_single, int bc, bool mixed) {
    return (g.toep && n_fill_single > 0 && !mixed) ? std::min(1.0, (double)n_fill_single / bc) : 0.0;
}
// One column step.  class 0: the LDS-DMA kernel of the fat steps (the dominant kernel, the roofline
// figure); class 12: its gradient-geometry instantiation (aux rows [I ; y'], <.., IDENT>: another
// kernel with its own flops, bytes and rate); class 9: the mixed-precision one; class 6: the
// direct-load kernel of the thin / full steps
inline Cost cost_col(const JobGeom &g, int bc, int jj, int mode, int k0_col, bool mixed, double lazy_frac) {
    const bool fat = mode == COL_FAT;
    const double k = (double)jj * NB;
    // rows that take part and the k-products they carry.  Gradient jobs (aux rows [I ; y']):
    // identity tile a joins from block column a on and its k-loop starts at 64 a — the kernels
    // skip the rest, so it is not counted either
    double rows = (double)(g.n0 - (jj + 1) * NB) + (double)g.naux;
    const double kc = k - k0_col;
    double rows_kc = rows * kc;
    if (g.aux_identity) {
        rows = (double)(g.n0 - (jj + 1) * NB) + (double)(g.naux - g.n0);   // main rows + y'
        rows_kc = rows * kc;
        for (int a = 0; a <= jj && a < g.nb0; ++a) {
            rows += NB;
            rows_kc += NB * std::max(0.0, k - std::max((double)k0_col, (double)a * NB));
        }
    }
    double fl = 2.0 * NB * rows_kc + rows * (double)NB * NB;
    double by = 8.0 * (rows_kc + NB * kc + 2.0 * rows * NB);
    if (fat) {  // + column jj+1 partial sums from the same rows
        fl += 2.0 * NB * rows_kc;
        by += 8.0 * (NB * k + 2.0 * rows * NB);
    }
    // Toeplitz jobs: the first step that touches a main tile of a single-table item reads 127
    // table entries instead of the stored tile (the sibling wave of the first row tile works
    // on the stored diagonal tile)
    if (lazy_frac > 0.0 && (fat || (mode == COL_FULL && jj == 0))) {
        const double rm = (double)(g.n0 - (jj + 1) * NB);
        by -= lazy_frac * 8.0 * NB * (rm + (fat ? std::max(0.0, rm - NB) : 0.0));
    }
    return {fat ? (mixed ? 9 : (g.aux_identity ? 12 : 0)) : 6, bc * fl, bc * by};
}
// the fill of a value job's chunk (Toeplitz jobs: single-table items store their diagonal tiles and
// aux rows only), of the aux rows alone (queries of a resident factor), of a gradient leaf's chunk
// (K's lower blocks, the y' tile row and the zero blocks (a, a - 1): the identity block of the aux
// rows is synthesised by the column kernels, not written)
inline Cost cost_fill(const JobGeom &g, int bc, int n_fill_single) {
    const double fill_elems = (double)bc * ((double)g.n0 * (g.n0 + NB) / 2.0 + (double)g.naux * g.n0) -
                              (g.toep ? (double)n_fill_single * ((double)g.n0 * (g.n0 - NB) / 2.0) : 0.0);
    return {4, 0.0, 8.0 * fill_elems};
}
inline Cost cost_fill_aux(const JobGeom &g, int bc) { return {4, 0.0, 8.0 * bc * (double)g.naux * g.n0}; }
inline Cost cost_fill_grad(const JobGeom &g, int bc, bool toep_path) {
    return {4, 0.0, 8.0 * bc * ((double)g.n0 * (g.n0 + NB) / 2.0 + (toep_path ? 1.0 : 2.0) * NB * (double)g.n0)};
}
inline Cost cost_gram(const JobGeom &g, int bc) {
    const double nrows_aux = (double)g.naux;
    return {2, bc * nrows_aux * nrows_aux * g.n0, bc * 8.0 * nrows_aux * g.n0};
}
// a resident factor's query: solve of the aux rows against block column jj, their update behind it
inline Cost cost_aux_solve(const JobGeom &g, int bc) {
    return {6, bc * (double)g.naux * (double)NB * NB, bc * 8.0 * 3.0 * (double)g.naux * NB};
}
inline Cost cost_aux_update(const JobGeom &g, int bc, int jj) {
    return {7, bc * (double)g.naux * 2.0 * NB * (double)(g.n0 - (jj + 1) * NB),
            bc * 8.0 * (g.n0 - (jj + 1) * NB) * (2.0 * (double)g.naux + NB)};
}
// gradient leaves: K^-1 = W W'; z'z and the backward sweep of the Toeplitz leaf's two aux rows (class
// 10 with the other backward sweeps of the library); the contractions
inline Cost cost_kinv(const JobGeom &g, int bc) {
    const double n3 = (double)g.n0 * g.n0 * g.n0;
    return {5, bc * n3 / 3.0, bc * 8.0 * 1.5 * (double)g.n0 * g.n0};
}
inline Cost cost_toep_quad(const JobGeom &g, int bc) { return {10, 0.0, bc * 8.0 * g.n0}; }
inline Cost cost_toep_back(int bc, int cc) {
    return {10, bc * 2.0 * 2.0 * NB * (double)(cc + 1) * NB,
            bc * 8.0 * ((double)NB * NB * (cc + 1) + 2.0 * 2.0 * NB * (cc + 1))};
}
inline Cost cost_toep_grad(const JobGeom &g, int bc) { return {11, 0.0, bc * 8.0 * 3.0 * (double)g.n0}; }
inline Cost cost_contract(const JobGeom &g, int bc) { return {11, 0.0, bc * 8.0 * 0.5 * (double)g.n0 * g.n0}; }
// ngp_factor_sample_long.  Block column jj of sigma's factorisation: the diagonal block is
// cost_diag; the rows below it carry k = 64 jj products each and a 64-wide solve, block row jj of L
// is read once per workgroup of four row blocks, a row block once in (k + 64 wide) and once out
inline Cost cost_ls_panel(const LongSampleGeom &g, int bc, int jj) {
    const double k = (double)jj * NB, rows = (double)(g.nb - jj - 1) * NB;
    const double wgs = (double)((g.nb - jj - 1 + 3) / 4);
    return {6, bc * (2.0 * NB * rows * k + rows * (double)NB * NB),
            bc * 8.0 * (rows * k + wgs * NB * k + 2.0 * rows * NB + (double)NB * NB)};
}
// X = mu + L Z of `paths` paths in `waves` tiles of 64 and `wgs` workgroups: a wave multiplies 64
// rows of L by its 64 paths over k = 64 (i + 1), summed over the row blocks K = mpad (mpad + 64) / 128;
// the rows of L are read once per workgroup, those of Z once per wave, a path is written once
inline Cost cost_ls_draw(const LongSampleGeom &g, double paths, double waves, double wgs) {
    const double K = (double)g.mpad * ((double)g.mpad + NB) / (2.0 * NB);
    return {2, 2.0 * waves * NB * NB * K, 8.0 * (wgs * NB * K + waves * NB * K + paths * (2.0 * g.m))};
}
// ngp_factor_sample_long_indep.  The pick of S mixtures of Pm components: a path writes its item
// and its component and walks its own mixture's weights alone
inline Cost cost_lsi_pick(const LongSampleGeom &g, int Pm) {
    return {4, 0.0, 8.0 * (double)g.N + 4.0 * (double)g.N * (double)Pm};
}
// the staged normals of `paths` paths (both forms): full rows of mpad doubles, written once
inline Cost cost_ls_normals(const LongSampleGeom &g, double paths) { return {4, 0.0, 8.0 * g.mpad * paths}; }

}  // namespace ngp

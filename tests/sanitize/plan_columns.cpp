// The block-column schedule of the column sweep (col_pair_offset, col_step, diag_ahead_waves,
// csrc/ngp_plan.h through ngp_internal.h) and the chunk rules beside it (splitk_eligible, diag_wave,
// kinv_route) at 9 items, printed for tests/test_geometry_cases_cpu.py, nb0 = 1 .. 12:
//   offset nb0 o
//   step   nb0 jj mode k0_col k0_diag ahead join
//   waves  jj w
//   route  nb0 invariant splitk diag_wave kinv        (kinv: of a gradient job of that many blocks)
// With the argument "small" it prints instead, for tests/test_small_grad_cases_cpu.py, the small_plan
// of a gradient job of n = 1 .. 256 points (refused: nbe = 0 and nothing after it):
//   small  n nbe ident nsweeps kind[nsweeps] colwave[nbe]
// Host code only (hipcc --cuda-host-only), the geometries set up as in plan_check.cpp.
#include <cstdio>
#include <cstring>

#include "../../nowcastautogp_amd/csrc/ngp_internal.h"

using namespace ngp;

static JobGeom value_geom(int nb0, int invariant) {
    JobGeom g{};
    g.n0 = nb0 * NB;
    g.nb0 = nb0;
    g.n_real = g.n0;
    g.naux = 39;
    g.naux_pad = NB;
    g.short_series = 1;
    g.invariant = invariant;
    return g;
}

static JobGeom grad_geom(int nb0, int invariant) {
    JobGeom g = value_geom(nb0, invariant);
    g.aux_identity = 1;
    g.naux = g.n0 + 1;
    g.naux_pad = g.n0 + NB;
    return g;
}

static void small_plans() {
    for (int n = 1; n <= SM_MAX_NB * NB; ++n) {
        JobGeom g = grad_geom((n + NB - 1) / NB, 0);
        g.n_real = n;
        SmallPlan pl{};
        if (!small_plan(g, &pl)) {
            printf("small %d 0\n", n);
            continue;
        }
        printf("small %d %d %d %d", n, pl.nbe, pl.ident, pl.nsweeps);
        for (int si = 0; si < pl.nsweeps; ++si) printf(" %d", pl.sw[si].main);
        for (int j = 0; j < pl.nbe; ++j) printf(" %d", (int)((pl.colwave >> (4 * j)) & 15));
        printf("\n");
    }
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "small")) {
        small_plans();
        return 0;
    }
    const int B = 9, NB_MAX = 12;
    printf("constants %d %d %d %d %d %d\n", NB, COL_FULL, COL_FAT, COL_THIN, DIAG_AHEAD_SPLIT_K, B);
    for (int nb0 = 1; nb0 <= NB_MAX; ++nb0) {
        const JobGeom g = value_geom(nb0, 0);
        printf("offset %d %d\n", nb0, col_pair_offset(g));
        for (int jj = 0; jj < nb0; ++jj) {
            const ColStepPlan st = col_step(g, jj);
            printf("step %d %d %d %d %d %d %d\n", nb0, jj, st.mode, st.k0_col, st.k0_diag, (int)st.ahead,
                   (int)st.join);
        }
    }
    for (int jj = 0; jj <= NB_MAX; ++jj) printf("waves %d %d\n", jj, diag_ahead_waves(jj));
    for (int nb0 = 1; nb0 <= NB_MAX; ++nb0)
        for (int inv = 0; inv < 2; ++inv) {
            const JobGeom g = value_geom(nb0, inv), gg = grad_geom(nb0, inv);
            printf("route %d %d %d %d %d\n", nb0, inv, (int)splitk_eligible(g, B, false, false),
                   (int)diag_wave(g, B), (int)kinv_route(gg, B));
        }
    return 0;
}

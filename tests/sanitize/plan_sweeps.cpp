// The sweeps small_plan (csrc/ngp_plan.h, through ngp_internal.h) gives every value-job geometry, printed for
// tests/test_value_cases_cpu.py: one line "n0 naux nsweeps" (0: refused, the column sweep takes it).
// Host code only (hipcc --cuda-host-only), the geometry set up as in plan_check.cpp.
#include <cstdio>

#include "../../nowcastautogp_amd/csrc/ngp_internal.h"

using namespace ngp;

int main() {
    printf("constants %d %d %d %d %d\n", SM_WAVES, SM_NSLOT, SM_MAX_PANEL, SM_MAX_SWEEPS, NGP_MAX_AUX);
    for (int n0 = 64; n0 <= 320; n0 += 64)
        for (int naux = 1; naux <= NGP_MAX_AUX; ++naux) {
            JobGeom g{};
            g.n0 = n0;
            g.nb0 = n0 / NB;
            g.n_real = n0;
            g.naux = naux;
            g.naux_pad = (naux + NB - 1) / NB * NB;
            g.short_series = 1;
            SmallPlan pl{};
            printf("%d %d %d\n", n0, naux, small_plan(g, &pl) ? pl.nsweeps : 0);
        }
    return 0;
}

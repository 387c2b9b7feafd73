// ngp_mixmap_plan.h — how the host cuts a date of ngp_mixture_crps_mapped into panels, from the
// record the scan kernel leaves (ngp_mixture_mapped_kernels.h).  Plain C++ without HIP: included by
// ngp_internal.h and, on its own, by tests/sanitize/mapped_stress.cpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace ngp {

constexpr int MIXMAP_TILE_PANELS = 16;     // panels per workgroup of the panel kernel
constexpr int MIXMAP_MAX_PANELS = 8192;    // per date: beyond it NGP_INFO_NOT_CONVERGED
constexpr double MIXMAP_PANEL_SD = 1.0;    // a panel is no wider than this many sd_min at first
constexpr double MIXMAP_DEFAULT_TOL = 1.0e-10;
enum { MIXMAP_REC_LO = 0, MIXMAP_REC_HI, MIXMAP_REC_SDMIN, MIXMAP_REC_ALO, MIXMAP_REC_AHI,
       MIXMAP_REC_X0, MIXMAP_REC_PSI0, MIXMAP_REC_CLIP, MIXMAP_REC_FLAG, MIXMAP_REC_BEYOND,
       MIXMAP_REC };
// one date at one panel width: n0 panels of width h0 from a0 (below x0), npanels - n0 of width h1
// from a1 (above x0)
struct MixMapPlan {
    int32_t date, npanels, n0, pad;
    double a0, h0, a1, h1;
};
// panels of a segment of length len at width <= wmax, before the cap (0 for an empty segment);
// any input, NaN and infinities included, gives a count in [0, 2 MIXMAP_MAX_PANELS]
inline int32_t mixmap_segment_panels(double len, double wmax) {
    if (!(len > 0.0)) return 0;
    const double r = std::ceil(len / wmax);              // wmax 0 or NaN: not a finite count
    if (!(r >= 1.0)) return 1;
    return r < 2.0 * MIXMAP_MAX_PANELS ? (int32_t)r : 2 * MIXMAP_MAX_PANELS;
}
// the first plan of a date from its record: both segments at MIXMAP_PANEL_SD sd_min, scaled down
// together where that is more than the cap allows
inline MixMapPlan mixmap_plan(int32_t date, const double *rec) {
    const double alo = rec[MIXMAP_REC_ALO], ahi = rec[MIXMAP_REC_AHI], x0 = rec[MIXMAP_REC_X0];
    const double wmax = MIXMAP_PANEL_SD * rec[MIXMAP_REC_SDMIN];
    int32_t n0 = mixmap_segment_panels(x0 - alo, wmax), n1 = mixmap_segment_panels(ahi - x0, wmax);
    if (!std::isfinite(alo) || !std::isfinite(ahi) || !std::isfinite(x0)) n0 = n1 = 0;
    if (n0 + n1 > MIXMAP_MAX_PANELS) {
        const double f = (double)MIXMAP_MAX_PANELS / ((double)n0 + (double)n1);
        const int32_t k0 = n0 ? std::max<int32_t>(1, (int32_t)(f * n0)) : 0;
        const int32_t k1 = n1 ? std::max<int32_t>(1, (int32_t)(f * n1)) : 0;
        n0 = k0;
        n1 = std::min<int32_t>(k1, MIXMAP_MAX_PANELS - n0);
    }
    MixMapPlan p{date, n0 + n1, n0, 0, alo, n0 ? (x0 - alo) / n0 : 0.0, x0, n1 ? (ahi - x0) / n1 : 0.0};
    return p;
}
// the same date at half the width; false where the cap does not allow it
inline bool mixmap_refine(MixMapPlan *p) {
    if (p->npanels < 1 || 2 * p->npanels > MIXMAP_MAX_PANELS) return false;
    p->n0 *= 2;
    p->npanels *= 2;
    p->h0 *= 0.5;
    p->h1 *= 0.5;
    return true;
}

}  // namespace ngp

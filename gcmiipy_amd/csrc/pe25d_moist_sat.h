// GCM_PE25D: the saturation routine of the moist physics (include/gcmcore.h, gcm_set_moist), host and device, for the
// units that evaluate it: pe25d_moist.hip (condensation, the host probe gcm_moist_saturation),
// pe25d_boundary_layer.hip (the saturation humidity of the surface) and pe25d_betts_miller.hip (the parcel's ascent and
// the reference humidity).  Every unit switches contraction off for the whole file ahead of this include, so every
// operation below is rounded on its own in each.
#pragma once
#include <cmath>

#include "gcm_math.h"

namespace gcm {

constexpr double kMoEps = kRd / kRv;
constexpr double kMoOneMinusEps = 1.0 - kRd / kRv;

struct MoistSat { double qs, dqs; int can; double pd; };   // pd = p_lev / den, the factor of dq_s (the pseudoadiabat's slope reads it)

// humidity.saturation_vapor_pressure (the Buck equation) and humidity.rh_to_mmr(1, p_lev, T) in the algebraically equal
// form q_s = eps e_s / (p_lev - (1 - eps) e_s), with dq_s / dT.  A cell can saturate iff e_s < p_lev; where it cannot
// (warm air at low pressure) q_s, dq_s and pd are 0 and nobody uses them
__host__ __device__ inline MoistSat moist_saturation(double T, double p_lev) {
    const double tc = T - 273.15;
    const double a = 18.678 - tc / 234.5;
    const double d = 257.14 + tc;
    const double b = tc / d;
    const double es = (0.61121 * 1000.0) * exp(a * b);
    MoistSat r{0.0, 0.0, es < p_lev ? 1 : 0, 0.0};
    if (!r.can) return r;
    const double den = p_lev - kMoOneMinusEps * es;
    r.qs = (kMoEps * es) / den;
    const double dlne = (a * 257.14) / (d * d) - tc / (234.5 * d);
    r.pd = p_lev / den;
    r.dqs = (r.qs * r.pd) * dlne;
    return r;
}

}  // namespace gcm

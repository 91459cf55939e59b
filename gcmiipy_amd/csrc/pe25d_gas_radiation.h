// GCM_PE25D, grey radiation that absorbs by water vapour and CO2 (grey_solar.py:192-320, clouds off: c = 0): the column
// routine, one text for the kernel (pe_gas_radiation_kernel) and the host probe (gcm_gas_radiation_columns), both in
// pe25d_gas_radiation.hip.  The contract: include/gcmcore.h.
//
// Every operation is float64 and rounded on its own, in the order written here: the unit that includes this header is
// built with contraction off (#pragma clang fp contract(off) ahead of the include, the Makefile's honor-pragmas mode).
#pragma once
#include <cmath>
#include <hip/hip_runtime.h>

#include "gcm_math.h"

namespace gcm {

constexpr double kGasSb = 5.67e-8, kGasCg = 1.13e6;   // constants.py:71,25
constexpr double kGasMco2 = 44.01, kGasMd = 28.97;    // constants.py: M_CO2, Md, g / mol

// the parameters of a launch: the weights, m^2 / kg, the CO2 mass mixing ratio co2_vmr M_CO2 / Md, the ground's albedo
// and `same`: both weight pairs are equal, so that the short wave's power of a level is the long wave's
struct GasPar {
    double k_h2o_lw, k_co2_lw, k_h2o_sw, k_co2_sw, co2, a_g;
    int same;
};

// what the caller hands in for level k: tp = p sig + ptop, dp = p dsig, the true temperature and q as stored; ex is the
// caller's own (the kernel: the Exner factor tt was formed with, for the way back to theta) and is handed on to out()
struct GasLevelIn { double tp, dp, tt, q, ex; };
// what a level is to either scan: Cp rho depth, the long-wave emissivity 1 - 10^-a_lw, the short wave's 1 - 10^-a_sw
// (sw: asked for) and the emission sb tt^4 e_lw
struct GasLevel { double heat, e_lw, a_sw1, E; };
// the column's words: SC is the caller's; SW_SFC = (1 - a_g) SWd[0], LW_DOWN = LWd[0], LW_UP = U_s, OLR = LWu[L]
struct GasColumn { double sw_sfc, lw_down, lw_up, olr, dt_ground; };

__host__ __device__ inline GasLevel gas_level(const GasPar &g, const GasLevelIn &in, bool sw) {
    const double qc = fmax(in.q, 0.0);
    const double rho = in.tp / (kRd * in.tt);
    const double depth = in.dp / (rho * kG);
    GasLevel v;
    const double a_lw = 0.0 + qc * rho * depth * g.k_h2o_lw + g.co2 * rho * depth * g.k_co2_lw;
    v.e_lw = 1 - exp10(-a_lw);
    v.a_sw1 = 0.0;
    if (sw) {
        if (g.same) {
            v.a_sw1 = v.e_lw;
        } else {
            const double a_sw = 0.0 + qc * rho * depth * g.k_h2o_sw + g.co2 * rho * depth * g.k_co2_sw;
            v.a_sw1 = 1 - exp10(-a_sw);
        }
    }
    const double t2 = in.tt * in.tt;
    v.E = kGasSb * (t2 * t2) * v.e_lw;
    v.heat = kCp * rho * depth;
    return v;
}

// The column, two scans.  The long wave absorbed from below is needed by a sum the top-down scan finishes, so the
// bottom-up scan goes first and parks one value per level (park(k) is a reference to the caller's storage); the
// top-down scan forms the level again (lev(k) is called twice per level) and hands the finished tendency to
// out(k, dt_air, in), in the order abs_k = (SW + LW from above) + LW from below of the reference
template <class Lev, class Park, class Out>
__host__ __device__ inline GasColumn gas_column(int L, const GasPar &g, double SC, double gt, Lev lev, Park park, Out out) {
    GasColumn c;
    const double g2 = gt * gt;
    c.lw_up = kGasSb * (g2 * g2);
    double up = c.lw_up;
    for (int k = 0; k < L; ++k) {                           // bottom-up: LWu[0] = U_s
        const GasLevel v = gas_level(g, lev(k), false);
        const double ab = up * v.e_lw;
        park(k) = ab;
        up = up - ab + v.E;
    }
    c.olr = up;
    double sw = SC, down = 0.0;
    for (int k = L - 1; k >= 0; --k) {                      // top-down: SWd[L] = SC, LWd[L] = 0
        const GasLevelIn in = lev(k);
        const GasLevel v = gas_level(g, in, true);
        double ab = sw * v.a_sw1;
        sw = sw - ab;
        const double ab_lw = down * v.e_lw;
        ab = ab + ab_lw;
        down = down - ab_lw + v.E;
        ab = ab + park(k);
        out(k, (ab - 2 * v.E) / v.heat, in);
    }
    c.sw_sfc = (1 - g.a_g) * sw;
    c.lw_down = down;
    const double gain = c.sw_sfc + c.lw_down;
    c.dt_ground = (gain - c.lw_up) / kGasCg / (.1);
    return c;
}

// cos of the zenith angle: solar_zenith_angle, grey_solar.py:40-46, cut off at the horizon
__host__ __device__ inline double gas_cos_zenith(double sinlat, double coslat, double sin_d, double cos_d, double point_angle) {
    return fmax(sinlat * sin_d + coslat * cos_d * cos(point_angle), 0.0);
}

}  // namespace gcm

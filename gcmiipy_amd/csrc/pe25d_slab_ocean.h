// GCM_PE25D, slab mixed-layer ocean: the cell routine, one text for the kernel (pe_slab_ocean_kernel) and the host probe
// (gcm_slab_ocean_cells), both in pe25d_slab_ocean.hip.  The contract: include/gcmcore.h.
//
// Every operation is float64 and rounded on its own, in the order written here: the unit that includes this header is
// built with contraction off (#pragma clang fp contract(off) ahead of the include, the Makefile's honor-pragmas mode).
#pragma once
#include <hip/hip_runtime.h>

namespace gcm {

// the flux words of one cell, GCM_SLAB_WORDS of them in the order of the GCM_SLAB_* indices
struct SlabWords { double sc, sw_sfc, lw_down, lw_up, olr, sh_j, evap_kg; };
struct SlabCell { double gt, E4; };

//   R  = (S + B) - U_s;  E1 = dt R;  E2 = E1 - SH_J;  E3 = E2 - Lv EVAP_KG;  E4 = E3 + dt Q;  gt' = gt + E4 / C
// C = +inf: E4 / C = 0 and gt + 0 keeps gt's bits (a cell held at its prescribed temperature)
__host__ __device__ inline SlabCell slab_cell(double gt, double C, double dt, double Lv, const SlabWords &w, double Q) {
    const double R = (w.sw_sfc + w.lw_down) - w.lw_up;
    const double E1 = dt * R;
    const double E2 = E1 - w.sh_j;
    const double E3 = E2 - Lv * w.evap_kg;
    SlabCell c;
    c.E4 = E3 + dt * Q;
    c.gt = gt + c.E4 / C;
    return c;
}

// what one application adds to the GCM_SLAB_SUMS sums of a cell, in their order; gt1: the cell's new temperature
__host__ __device__ inline void slab_sums(double *out, double dt, double Lv, const SlabWords &w, double Q, double gt1) {
    out[0] = dt * w.sc;
    out[1] = dt * w.sw_sfc;
    out[2] = dt * w.lw_down;
    out[3] = dt * w.lw_up;
    out[4] = dt * w.olr;
    out[5] = w.sh_j;
    out[6] = Lv * w.evap_kg;
    out[7] = dt * Q;
    out[8] = dt * gt1;
    out[9] = dt * (gt1 * gt1);
}

}  // namespace gcm

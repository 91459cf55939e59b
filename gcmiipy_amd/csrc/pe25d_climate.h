// Zonal-mean climatology of GCM_PE25D (gcm_set_climate): host-visible interface of pe25d_climate.hip's kernel, used by
// that unit's own host code.  The contract, the moment table and the reduction order: include/gcmcore.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/gcmcore.h"

namespace gcm {

struct ClimateArgs {
    const void *p;                // [j][i] in the handle's real type, interior row 0
    const void *u, *v, *t;        // [j][k][i], interior row 0 (a band: v's north ghost row is row -1)
    const double *sig;            // [L] float64 mid-level sigma
    const double *exner_tab;
    double *m3;                   // [GCM_CLIM_WORDS3][L][H] float64 sums
    double *m2;                   // [GCM_CLIM_WORDS2][H]
    double ptop;
    int W, H, L;
    int wrap;                     // 1: row -1 is row H - 1 (single domain)
    int nseg;                     // gridDim.y: segment s walks levels [s L / nseg, (s + 1) L / nseg)
};

size_t climate_lds_bytes(int W);  // dynamic LDS of a launch
// one sample of the state `a` points to, added to a.m3 / a.m2, on `s`; cus: the device's compute units (sizes nseg)
void launch_climate(ClimateArgs a, bool f32, int cus, hipStream_t s);

}  // namespace gcm

// Zonal wavenumber spectra of GCM_PE25D (gcm_set_spectra): host-visible interface of pe25d_spectra.hip's kernel, used by
// that unit's own host code.  The contract and the word table: include/gcmcore.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/gcmcore.h"
#include "fft_lds.h"

namespace gcm {

constexpr int kSpThreads = 512;      // two workgroups of eight waves a CU at W = 1440: four waves per SIMD
constexpr int kSpBatch = 2;           // 512-column chunks requested together, then packed in order
constexpr int kSpMaxPerThread = 4;    // wavenumbers a thread holds across the second transform, at the most
constexpr size_t kSpLdsCap = 160 * 1024;   // a workgroup's LDS on gfx950

struct SpectraArgs {
    const void *p;                // [j][i] in the handle's real type, interior row 0
    const void *u, *v, *t;        // [j][k][i], interior row 0 (a band: v's north ghost row is row -1)
    const double *sig;            // [L] float64 mid-level sigma
    const double *exner_tab;
    const double2 *tw;            // [W] float64 twiddles exp(-2 pi i n / W)
    double *s;                    // [GCM_SPEC_WORDS][L][H][M] float64 sums
    double ptop;
    FftPlan plan;                 // the generic mixed-radix plan of W
    int W, H, L, M;               // M = mmax + 1
    int wrap;                     // 1: row -1 is row H - 1 (single domain)
    int nseg;                     // gridDim.y: segment s walks levels [s L / nseg, (s + 1) L / nseg)
};

size_t spectra_lds_bytes(int W);  // dynamic LDS of a launch
// level segments of a launch over H rows: some four workgroups a CU; the sums do not depend on it
int spectra_nseg(int H, int L, int cus);
// exp(-2 pi i n / W), n = 0 .. W - 1, in float64 from angles reduced to an octant in integers
void spectra_twiddles(int W, double2 *tw);

}  // namespace gcm

// Launch geometry of the GCM_PE25D phases whose grid depends on the rows, the row length and the chip's compute units:
// the Held-Suarez forcing, the moist physics, the climatology's sample and the tracers' forcing.  Host arithmetic only,
// no device: hs_launch, mo_launch, launch_climate and launch_tracer_force take their numbers from here, and so does the
// query gcm_pe25d_phase_geometry / gcm_pe25d_phase_plan (include/gcmcore.h), so that the query cannot drift from the
// launch.  The kernels read the constants below from here too.
#pragma once
#include <algorithm>

#include "../../include/gcmcore.h"

namespace gcm {

constexpr int kHsThreads = 256;
constexpr int kHsBatch = 4;          // levels requested together, then advanced in order
constexpr int kMoThreads = 256;
constexpr int kMoBatch = 4;          // levels requested together, then advanced in order
constexpr int kClThreads = 256;
constexpr int kClBatch = 3;          // 256-column chunks requested together, then added in order
constexpr int kTfThreads = 256;
// the most workgroups per entry: 8 per CU; a 1440 x 720 x 24 field in fp64 is then 24 passes of 8 MiB
constexpr int kTfGroupsMax = 2048;

// segment s of nseg marches levels [s L / nseg, (s + 1) L / nseg)
inline int phase_seg_level0(int seg, int L, int nseg) { return (int)((long)seg * L / nseg); }

// Held-Suarez and moist physics: grid (column blocks, rows, level segments).  split: the levels are split over the grid
// where the rows alone do not fill the chip (a band's ghost rows, a small band); else whole columns
struct PhaseColumnGrid { int xb, nrows, nseg; };
inline PhaseColumnGrid phase_column_grid(int W, int nrows, int L, int cus, int threads, bool split) {
    PhaseColumnGrid g{(W + threads - 1) / threads, nrows, 1};
    const long blocks = (long)g.xb * nrows;
    if (split && blocks > 0) g.nseg = (int)std::min<long>(L, std::max<long>(1, (2L * cus + blocks - 1) / blocks));
    return g;
}

// the climatology's sample: grid (rows, level segments); the levels are split over the grid until some eight
// workgroups a CU are in flight
inline int phase_climate_nseg(int H, int L, int cus) { return (int)std::min<long>(L, std::max<long>(1, (8L * cus + H - 1) / H)); }
// iterations of a level's chunk loop: kClBatch chunks of kClThreads columns each
inline int phase_climate_chunks(int W) { return (W + kClBatch * kClThreads - 1) / (kClBatch * kClThreads); }

// the tracers' forcing: workgroups per entry for a run of n elements, 16 bytes (V elements) per lane
inline long phase_tracer_force_groups(long n, int elem_bytes) {
    const long V = 16 / elem_bytes;
    return std::min<long>(kTfGroupsMax, std::max<long>(1, (n / V + kTfThreads - 1) / kTfThreads));
}

// gcm_pe25d_phase_geometry
inline int pe25d_phase_geometry(int phase, int W, int rows, int L, int cus, int elem_bytes, int accumulate, int *out, int nout) {
    if (W < 1 || rows < 1 || L < 1 || cus < 1 || (elem_bytes != 4 && elem_bytes != 8) || !out || nout < GCM_PHASE_PLAN_WORDS)
        return GCM_ERR_ARG;
    for (int n = 0; n < GCM_PHASE_PLAN_WORDS; ++n) out[n] = 0;
    int nseg = 0;
    switch (phase) {
    case GCM_PHASE_HELD_SUAREZ:
    case GCM_PHASE_MOIST: {
        const bool hs = phase == GCM_PHASE_HELD_SUAREZ;
        const PhaseColumnGrid g = phase_column_grid(W, rows, L, cus, hs ? kHsThreads : kMoThreads, hs || !accumulate);
        out[0] = g.xb; out[1] = g.nrows; out[2] = nseg = g.nseg;
        break;
    }
    case GCM_PHASE_CLIMATE:
        out[0] = rows; out[1] = nseg = phase_climate_nseg(rows, L, cus);
        out[4] = phase_climate_chunks(W);
        break;
    case GCM_PHASE_TRACER_FORCING: {
        const long n = (long)rows * L * W, V = 16 / elem_bytes;
        const long groups = phase_tracer_force_groups(n, elem_bytes), pass = groups * kTfThreads;
        out[0] = (int)groups;
        out[1] = (int)std::max<long>(1, (n / V + pass - 1) / pass);
        return GCM_OK;
    }
    default:
        return GCM_ERR_ARG;
    }
    // the fewest and the most levels a segment marches
    int lo = L, hi = 0;
    for (int s = 0; s < nseg; ++s) {
        const int n = phase_seg_level0(s + 1, L, nseg) - phase_seg_level0(s, L, nseg);
        lo = std::min(lo, n); hi = std::max(hi, n);
    }
    out[phase == GCM_PHASE_CLIMATE ? 2 : 3] = lo;
    out[phase == GCM_PHASE_CLIMATE ? 3 : 4] = hi;
    return GCM_OK;
}

}  // namespace gcm

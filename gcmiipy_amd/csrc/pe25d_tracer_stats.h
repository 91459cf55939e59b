// Device monitor of the passive tracers (and q) of GCM_PE25D: host-visible interface of pe25d_tracer_stats.hip,
// used by pe25d_tracers.hip (pe25d_tracer_stats).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/gcmcore.h"

namespace gcm {

// Fields are [j][k][i] in the handle's real type, addressed from own row 0 (a band's ghost rows lie outside
// [0, H) and are never read); p is [j][i].  Field f < ntr is tr + f * tstride, field f == ntr is q.
struct TracerStatsArgs {
    const void *tr;          // tracer 0 of the set asked for (null with ntr == 0)
    long tstride;            // elements between two tracers
    const void *q;           // q of the same state set (read only as field ntr)
    const void *p;           // p of the same state set
    const double *dsig;      // [L], float64 for either real type
    double *part;            // [nf][groups][GCM_TRACER_STATS_WORDS]
    double *out;             // [nf][GCM_TRACER_STATS_WORDS]
    int ntr, nf, W, H, L;
};

// the workgroups of one field: a function of the handle's size alone, so that the order of every sum is too
int tracer_stats_groups(int H, int W);
// two launches on `s`: the workgroups' records to a.part, then their fold in index order to a.out
void launch_tracer_stats(const TracerStatsArgs &a, bool f32, hipStream_t s);

}  // namespace gcm

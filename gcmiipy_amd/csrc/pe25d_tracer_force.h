// Forcing of the passive tracers of GCM_PE25D (gcm_set_tracer_forcing): host-visible interface of
// pe25d_tracer_force.hip, used by pe25d_tracers.hip (launch_tracers).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/gcmcore.h"

namespace gcm {

// One forced tracer.  c, emis and mask all point at own row 0 of fields in the tracers' device layout [j][k][i]
// (emis in T, mask in bytes, own rows only; either may be null: the field is then never read).  The wide path needs
// c and emis equally placed within 16 bytes, and mask placed like c's element index within a vector; the registration
// allocates them so, and the kernel falls back to single elements where they are not.
template <typename T>
struct TracerForceEntryT {
    T *c;
    const T *emis;
    const unsigned char *mask;
    T source, fac, pin;      // fac = T(exp(-decay dt))
};

// The compact list of the forced tracers (blockIdx.y = the entry) and the two runs of own rows of the corrector
// launch they follow: rows [r0, r1) and [rb0, rb1) of a field are off* .. off* + n* elements from own row 0.
template <typename T>
struct TracerForceArgsT {
    TracerForceEntryT<T> e[GCM_MAX_TRACERS];
    long off0, n0, off1, n1;
    T dt;
};

// one launch on `s`, grid (workgroups, entries); nothing with entries == 0 or no elements
template <typename T>
void launch_tracer_force(const TracerForceArgsT<T> &a, int entries, hipStream_t s);

}  // namespace gcm

// Implicit vertical mixing of the passive tracers of GCM_PE25D (gcm_set_tracer_mixing): host-visible interface of
// pe25d_tracer_mix.hip, used by pe25d_tracers.hip (launch_tracers) and gcmcore.hip (gcm_tracer_mixing_coeffs).
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/gcmcore.h"

namespace gcm {

// gcm_tracer_mixing_coeffs: the float64 coefficients lo, w, g [L] of the backward-Euler column solve from dsig [L],
// K [L - 1] and dtd, every operation rounded on its own, in the order include/gcmcore.h gives.  Needs no device.
// GCM_ERR_ARG (and *err) for L < 2, a null pointer, a non-finite or negative K; nothing is written then
int tracer_mixing_coeffs(int L, const double *dsig, const double *k, double dtd, double *lo, double *w, double *g, std::string *err);

// The compact list of the mixed tracers (blockIdx.y = the entry) and the two runs of own rows of the corrector launch
// they follow: rows [j0, j0 + n0) and [jb0, jb0 + n1).  c[e] points at own row 0 of entry e in the tracers' device
// layout [j][k][i]; tab holds, per entry, lo [L], w [L], g [L] in T: constant for the launch, read through scalar loads
template <typename T>
struct TracerMixArgsT {
    T *c[GCM_MAX_TRACERS];
    const T *tab;
    int W, L, j0, n0, jb0, n1;
};

// one launch on `s`, grid (workgroups, entries); nothing with entries == 0 or no rows.  L <= 24 and L <= 40 keep the
// column in registers (one read and one write of each cell); above, y is written into c on the way up and read again
// on the way down: the same arithmetic and bits
template <typename T>
void launch_tracer_mix(const TracerMixArgsT<T> &a, int entries, hipStream_t s);

// the largest level count whose column stays in registers
constexpr int kTmLevelsMax = 40;

// n <= kTmFillMax values of T into dst[0 .. n) by one small launch on `s`: the values travel in the kernel's
// arguments, which the runtime copies at the call, so the write is in stream order and the host array is free at once
constexpr int kTmFillMax = 256;
template <typename T>
void launch_tracer_mix_fill(T *dst, const T *values, int n, hipStream_t s);

}  // namespace gcm

// GCM_PE25D, sigma -> pressure interpolation of a column (gcm_plev_columns, gcm_plev_fields, gcm_set_plev_climate): the
// column rule as routines the two kernels of pe25d_plev.hip and the host build share, the kernels' arguments and the
// constants of their shape.  pe25d_plev.hip switches contraction off for the whole file ahead of this header (#pragma
// clang fp contract(off), -ffp-contract=fast-honor-pragmas): a column's values are the same bits in either kernel and
// on the host.  The contract: include/gcmcore.h.
//
// Levels run k = 0 (bottom) .. L - 1 (top); pl[k] = sig[k] p + ptop decreases strictly with k where p > 0.  Targets
// P[n] are full pressure in Pa, strictly decreasing: they run the way k does.  Everything is float64, every operation
// rounded on its own; the division is the compiler's correctly rounded one.
#pragma once
#include <cmath>

#include <hip/hip_runtime.h>

#include "../../include/gcmcore.h"

namespace gcm {

// ---------------------------------------------------------------- the column rule (host and device: one set of routines)
// target P of a column whose bottom and top mid-levels lie at pl0 = pl[0] and plt = pl[L - 1]: valid iff plt <= P <= pl0,
// no extrapolation.  plt < pl0 fails for p <= 0 (the levels do not decrease) and for a NaN p (every comparison fails):
// such a column has no valid target
__host__ __device__ inline bool plev_valid(double pl0, double plt, double P) { return plt < pl0 && plt <= P && P <= pl0; }

// the bracket of a valid target is the largest k in 0 .. L - 2 with pl[k] >= P.  Where the levels decrease that is the
// one k with pl[k] >= P > pl[k + 1], or, for the top bracket (k = L - 2: `last`), pl[k] >= P >= pl[k + 1]: a march from
// the bottom recognises it from the two levels it holds
__host__ __device__ inline bool plev_in_bracket(double plk, double plk1, bool last, double P) {
    return plk >= P && (last ? plk1 <= P : plk1 < P);
}

// the weight of level k + 1; 0 exactly where P = pl[k]
__host__ __device__ inline double plev_weight(double plk, double plk1, double P) { return (plk - P) / (plk - plk1); }

// (1 - w) x[k] + w x[k + 1]: w = 0 returns x[k] and w = 1 returns x[k + 1] exactly (a NaN in the other level aside: NaN
// propagates, and never decides validity)
__host__ __device__ inline double plev_interp(double w, double xk, double xk1) { return (1.0 - w) * xk + w * xk1; }

// one column, one quantity, all targets: pl, x [L], P [N] -> out, valid [N]; out is left alone where a target is invalid
inline void plev_column(int L, int N, const double *pl, const double *x, const double *P, double *out, int *valid) {
    for (int n = 0; n < N; ++n) {
        valid[n] = plev_valid(pl[0], pl[L - 1], P[n]) ? 1 : 0;
        if (!valid[n]) continue;
        int k = L - 2;
        while (k > 0 && !(pl[k] >= P[n])) --k;
        out[n] = plev_interp(plev_weight(pl[k], pl[k + 1], P[n]), x[k], x[k + 1]);
    }
}

// targets as every entry point takes them: 1 <= N <= GCM_PLEV_MAX, finite, positive, strictly decreasing
inline bool plev_targets_ok(int N, const double *P) {
    if (!P || N < 1 || N > GCM_PLEV_MAX) return false;
    for (int n = 0; n < N; ++n)
        if (!std::isfinite(P[n]) || !(P[n] > 0.0) || (n > 0 && !(P[n] < P[n - 1]))) return false;
    return true;
}

// ---------------------------------------------------------------- the kernels' shape
constexpr int kPlThreads = 256;      // the climatology's: the reduction order of a row is its order (kClThreads)
constexpr int kPlWaves = kPlThreads / 64;
constexpr int kPlSegTargets = 4;     // targets of a workgroup of the sample: 13 sums each in a thread's registers
constexpr int kPlFieldQ = 5;         // uc, vc, theta, T, q

inline int plev_nseg(int N) { return (N + kPlSegTargets - 1) / kPlSegTargets; }
inline int plev_chunks(int W) { return (W + kPlThreads - 1) / kPlThreads; }
size_t plev_lds_bytes();             // the sample's: the Exner table and two buffers of the waves' sums (pe25d_plev.hip)

struct PlevArgs {
    const void *p;                // [j][i] in the handle's real type, interior row 0
    const void *u, *v, *t, *q;    // [j][k][i], interior row 0 (a band: v's north ghost row is row -1)
    const double *sig;            // [L] float64 mid-level sigma
    const double *exner_tab;
    const double *P;              // [N] targets, device
    double *s;                    // the sample: [GCM_PLEV_WORDS][N][H] float64 sums
    double *out;                  // the maps: [kPlFieldQ][N][H][W]
    int32_t *valid;               // the maps: [N][H][W], may be null
    double fill;                  // the maps: what an invalid entry holds
    double ptop;
    int W, H, L, N;
    int wrap;                     // 1: row -1 is row H - 1 (single domain)
};

}  // namespace gcm

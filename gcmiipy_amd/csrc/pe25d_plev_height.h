// GCM_PE25D, geopotential height on pressure levels (gcm_plev_height_columns, gcm_plev_height, gcm_set_plev_maps): the
// column rule as one march that the kernel of pe25d_plev_height.hip and the host build share, the kernel's arguments and
// the constants of its shape.  pe25d_plev_height.hip switches contraction off for the whole file ahead of this header
// (#pragma clang fp contract(off), -ffp-contract=fast-honor-pragmas): a column's Z is the same bits in the map call, in
// the sample and on the host.  The contract: include/gcmcore.h.
//
// Levels, targets, validity and bracket are pe25d_plev.h's (plev_valid, plev_in_bracket, plev_targets_ok).  Everything
// is float64, storage values widened exactly, every operation rounded on its own; the divisions are the compiler's
// correctly rounded ones (the model's own geopotential takes rcp for 1 / rho: its phi agrees to rounding, not bit for
// bit).  Pi is the kernels' own Exner routine (gcm_math.h: one routine for host and device).
//
// The mid-level geopotential is the model's (pe_geopot_kernel; compute_geopotential of the reference), in its order:
//   rho[k] = pl[k] / (Rd (theta[k] Pi[k]))            s1[k] = ((sig[k] p) / rho[k]) dsig[k]
//   stp[k] = (Cp (0.5 (theta[k] + theta[k + 1]))) (Pi[k] - Pi[k + 1]),  k + 1 = L wraps to 0, as the model has it
//   s2[k]  = sigt[k] stp[k]
//   phi[0] = (sum_k (s1[k] - s2[k]), k ascending from 0.0) + hmG        hmG = heightmap G of the column
//   phi[k] = phi[k - 1] + stp[k - 1]
// In bracket k the height continues the model's hydrostatic relation inside the layer, linear in Pi and not in p:
//   Z[n] = (phi[k] + (Cp (0.5 (theta[k] + theta[k + 1]))) (Pi(pl[k]) - Pi(P[n]))) / G
// A target that sits exactly on pl[k] returns phi[k] / G exactly (the difference of the two Pi is 0.0); one that sits on
// pl[k + 1] of its bracket (the top mid-level only, plev_in_bracket) returns (phi[k] + stp[k]) / G = phi[k + 1] / G, the
// same operation that forms phi[k + 1]: a level's height has the same bits from either of its two brackets.
// No extrapolation under the ground or above the top mid-level.  NaN in theta propagates and never decides validity; a
// column with p <= 0 or a NaN p has no valid target.
#pragma once
#include "gcm_math.h"
#include "pe25d_plev.h"

namespace gcm {

// ---------------------------------------------------------------- the column rule (host and device: one march)
// (Cp (0.5 (theta[k] + theta[k + 1]))): the factor stp[k] and the continuation inside bracket k share
__host__ __device__ inline double plev_height_layer(double thk, double thk1) { return kCp * (0.5 * (thk + thk1)); }

// s1[k] - s2[k]
__host__ __device__ inline double plev_height_term(double sigk, double dsigk, double sigtk, double p, double plk, double thk,
                                                   double pik, double stp) {
    const double rho = plk / (kRd * (thk * pik));
    const double s1 = ((sigk * p) / rho) * dsigk;
    return s1 - sigtk * stp;
}

// One column, all targets.  lev: sig [L], dsig [L], sigt [L]; tab: the Exner table; piP [N]: exner(P[n], tab), the same
// for every column; th(k): theta of level k, widened.  Two passes over theta: phi[0] is a sum over every level, so no
// height is known before the whole column was seen; the second pass carries phi upward from the bottom and stops behind
// the bracket of the last valid target.  For target n in order: hit(n, k, Z, plk, plk1, thk, thk1, pik, pik1) where it
// is valid, k its bracket, or miss(n).  Targets decrease: the invalid ones under the ground come first, the ones above
// the top mid-level last.  CHUNK: the levels of theta a pass requests at a time, all of them before the first is used --
// one memory latency a chunk, not one a level; it changes the order of the loads only, never a bit of the result
template <int CHUNK, class Th, class Hit, class Miss>
__host__ __device__ inline void plev_height_march(int L, int N, const double *P, const double *piP, double p, double ptop,
                                                  const double *lev, double hmG, const double *tab, Th th, Hit hit, Miss miss) {
    const double *sig = lev, *dsig = lev + L, *sigt = lev + 2 * L;
    const double pl0 = sig[0] * p + ptop, plt = sig[L - 1] * p + ptop;
    int n = 0;
    // (the targets under the ground; a column with p <= 0 or a NaN p: all of them, here and behind the march)
    while (n < N && !plev_valid(pl0, plt, P[n]) && !(P[n] < plt)) miss(n++);
    if (n < N && plev_valid(pl0, plt, P[n])) {
        const double th0 = th(0), pi0 = exner(pl0, tab);
        double acc = 0.0, thk = th0, pik = pi0, plk = pl0;
        for (int k0 = 0; k0 < L; k0 += CHUNK) {
            double up[CHUNK];                               // theta of the levels k0 + 1 .. k0 + CHUNK
#pragma unroll
            for (int c = 0; c < CHUNK; ++c) up[c] = k0 + c + 1 < L ? th(k0 + c + 1) : th0;
#pragma unroll
            for (int c = 0; c < CHUNK; ++c) {
                const int k = k0 + c;
                if (k >= L) break;
                const bool top = k + 1 == L;
                const double plk1 = top ? pl0 : sig[k + 1] * p + ptop;
                const double thk1 = up[c], pik1 = top ? pi0 : exner(plk1, tab);
                const double stp = plev_height_layer(thk, thk1) * (pik - pik1);
                acc = acc + plev_height_term(sig[k], dsig[k], sigt[k], p, plk, thk, pik, stp);
                thk = thk1; pik = pik1; plk = plk1;
            }
        }
        double phi = acc + hmG;                                // phi[0]
        thk = th0; pik = pi0; plk = pl0;
        for (int k0 = 0; k0 + 1 < L && n < N && plev_valid(pl0, plt, P[n]); k0 += CHUNK) {
            double up[CHUNK];
#pragma unroll
            for (int c = 0; c < CHUNK; ++c) up[c] = k0 + c + 1 < L ? th(k0 + c + 1) : th0;
#pragma unroll
            for (int c = 0; c < CHUNK; ++c) {
                const int k = k0 + c;
                if (!(k + 1 < L && n < N && plev_valid(pl0, plt, P[n]))) break;
                const double plk1 = sig[k + 1] * p + ptop;
                const double thk1 = up[c], pik1 = exner(plk1, tab);
                const double layer = plev_height_layer(thk, thk1);
                while (n < N && plev_valid(pl0, plt, P[n]) && plev_in_bracket(plk, plk1, k + 2 == L, P[n])) {
                    hit(n, k, (phi + layer * (pik - piP[n])) / kG, plk, plk1, thk, thk1, pik, pik1);
                    ++n;
                }
                phi = phi + layer * (pik - pik1);              // phi[k + 1]
                thk = thk1; pik = pik1; plk = plk1;
            }
        }
    }
    // (the targets above the top mid-level)
    for (; n < N; ++n) miss(n);
}

// ---------------------------------------------------------------- the kernel's shape
constexpr int kPhHostChunk = 8;      // CHUNK of the host build
// CHUNK of the kernel by real type, as measured at 1440 x 720 x 24 (profiles/plev_maps/README.md): float64 storage gains
// from eight levels in flight, float32 storage is fastest with one (158 vector registers instead of 198)
template <typename T> constexpr int plev_height_chunk() { return sizeof(T) == 8 ? 8 : 1; }
constexpr int kPhThreads = 256;      // one lane per column, 256 consecutive i of a row per workgroup

inline int plev_height_chunks(int W) { return (W + kPhThreads - 1) / kPhThreads; }

struct PlevHeightArgs {
    const void *p;                // [j][i] in the handle's real type, interior row 0
    const void *u, *v, *t, *q;    // [j][k][i], interior row 0 (a band: v's north ghost row is row -1); the maps read t only
    const void *hm;               // heightmap [Hg][W] in the handle's real type, global rows, or null
    const double *lev;            // sig [L], dsig [L], sigt [L], float64
    const double *exner_tab;
    const double *P;              // [N] targets, device
    double *s;                    // the sample: [GCM_PLEV_MAP_WORDS][N][H][W] float64 sums
    double *s2;                   // the sample: [GCM_PLEV_MAP_WORDS2][H][W]
    double *out;                  // the map call: Z [N][H][W]
    int32_t *valid;               // the map call: [N][H][W], may be null
    double fill;                  // the map call: what an invalid entry holds
    double ptop;
    int W, H, L, N;
    int row0;                     // the global row of own row 0 (the heightmap's)
    int wrap;                     // 1: row -1 is row H - 1 (single domain)
};

}  // namespace gcm

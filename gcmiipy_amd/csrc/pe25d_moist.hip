// GCM_PE25D, moist physics (gcm_set_moist, gcm_moist_step): large-scale condensation of the specific humidity q with
// latent heating of theta and immediate precipitation, and an optional moisture source at the level next to the surface,
// one launch per step behind the Held-Suarez forcing, the boundary layer and the convective adjustment.  The contract: include/gcmcore.h.
//
//   per cell (device, float64 for either storage type, rounded once to it):
//     p_lev = sig[k] p + ptop;  Pi = (p_lev / P0)^kappa (exner());  T = theta Pi;  (q_s, dq_s, can) = moist_saturation(T, p_lev)
//     can and q > q_s:  C = (q - q_s) / (1 + (Lv / Cp) dq_s);  q <- q - C;  theta <- theta + ((Lv / Cp) C) / Pi
//   per column:  P = sum_k C_k ((dsig[k] p) / G),  k = 0 .. L - 1 in order, from 0.0
//   level kb (largest sig), tau_e > 0, behind its condensation:  q_eq = rh_s q_s(theta_new Pi, p_lev);  x = dt / tau_e
//     can and q_eq > q:  q_new = (q + x q_eq) / (1 + x);  E = (q_new - q) ((dsig[kb] p) / G);  q <- q_new
//
// Every operation is rounded on its own: contraction is off for the whole file (the Makefile builds it with
// -ffp-contract=fast-honor-pragmas), host and device, so that a cell gets the same bits whichever launch -- a single
// domain's, a band's own rows', a neighbour's ghost rows', any split of the levels -- produces it, and the host probe
// gcm_moist_saturation evaluates the very routine the kernel calls.
//
// The state's layout is [j][k][i]: one lane owns the column (j, i), a wave is 64 consecutive i of one row, so the request
// of a level is one contiguous run.  Levels are requested kMoBatch at a time and advanced in order; p is read once per
// column, theta and q once per cell, and written where something condensed (q also where the surface moistened it).
// The precipitation is a register sum over the lane's own column: the fixed order costs nothing, one writer per
// accumulator word and launch, no atomics.  No LDS but the 2 KB Exner table.
#pragma clang fp contract(off)
#include "pe25d_host.h"
#include "pe25d_phase_geometry.h"
#include "pe25d_moist_sat.h"

namespace gcm {

// ---------------------------------------------------------------- saturation (host and device: one routine, pe25d_moist_sat.h)
int moist_check(const gcm_moist *mo, const char *fn, std::string *err) {
    const auto bad = [&](const char *what) { *err = std::string(fn) + ": " + what; return GCM_ERR_ARG; };
    if (!mo) return bad("no parameters");
    if (!std::isfinite(mo->Lv) || !std::isfinite(mo->tau_e) || !std::isfinite(mo->rh_s)) return bad("every parameter must be finite");
    if (!(mo->Lv > 0.0)) return bad("Lv must be > 0");
    if (mo->tau_e < 0.0) return bad("tau_e must be >= 0");
    if (!(mo->rh_s > 0.0 && mo->rh_s <= 1.0)) return bad("rh_s must lie in (0, 1]");
    return GCM_OK;
}

int moist_saturation_table(int n, const double *T, const double *p_lev, double *q_s, double *dq_s, int *can, std::string *err) {
    if (n < 0 || (n > 0 && (!T || !p_lev))) { *err = "gcm_moist_saturation: n must be >= 0, T and p_lev are required"; return GCM_ERR_ARG; }
    for (int i = 0; i < n; ++i) {
        const MoistSat r = moist_saturation(T[i], p_lev[i]);
        if (q_s) q_s[i] = r.qs;
        if (dq_s) dq_s[i] = r.dqs;
        if (can) can[i] = r.can;
    }
    return GCM_OK;
}

// ---------------------------------------------------------------- the kernel
// (kMoThreads, kMoBatch -- levels requested together, then advanced in order: pe25d_phase_geometry.h)
template <typename T>
struct MoArgsT {
    const T *p;                      // [j][i], interior row 0
    T *t, *q;                        // [j][k][i], interior row 0
    const double *sig, *dsig;        // [L]
    const double *exner_tab;
    double *precip, *evap;           // [H][W] own rows, or null: the launch accumulates nothing
    double ptop, lc, x, rh_s;        // Lv / Cp;  dt / tau_e, 0 where tau_e = 0 (no evaporation)
    int W, L, H, kb;
    int j0, n0, jb0, nrows;          // the rows of the launch: [j0, j0 + n0), then from jb0 on (a band's ghost rows: negative / >= H)
    int nseg;                        // gridDim.z: segment s marches levels [s L / nseg, (s + 1) L / nseg); 1 where the launch accumulates
};

// grid (column blocks, rows, level segments)
template <typename T>
__global__ __launch_bounds__(kMoThreads) void pe_moist_kernel(MoArgsT<T> a) {
    __shared__ double tab[kExnerTabDoubles];
    for (int n = threadIdx.x; n < kExnerTabDoubles; n += kMoThreads) tab[n] = a.exner_tab[n];
    __syncthreads();
    const int W = a.W, L = a.L;
    const int i = blockIdx.x * kMoThreads + threadIdx.x;
    const int r = (int)blockIdx.y;
    if (i >= W || r >= a.nrows) return;
    const int j = r < a.n0 ? a.j0 + r : a.jb0 + (r - a.n0);
    const int seg = (int)blockIdx.z;
    const int k0 = (int)((long)seg * L / a.nseg), k1 = (int)((long)(seg + 1) * L / a.nseg);
    const long c3 = (long)j * L * W + i;
    const double pc = (double)a.p[(long)j * W + i];
    double P = 0.0, E = 0.0;
    for (int k = k0; k < k1; k += kMoBatch) {
        T th[kMoBatch], qq[kMoBatch];
#pragma unroll
        for (int n = 0; n < kMoBatch; ++n) {
            const int kk = k + n;
            if (kk >= k1) break;
            const long o = c3 + (long)kk * W;
            th[n] = a.t[o];
            qq[n] = a.q[o];
        }
#pragma unroll
        for (int n = 0; n < kMoBatch; ++n) {
            const int kk = k + n;
            if (kk >= k1) break;
            const long o = c3 + (long)kk * W;
            const double pl = a.sig[kk] * pc + a.ptop;
            const double pi = exner(pl, tab);
            double theta = (double)th[n], q = (double)qq[n];
            MoistSat s = moist_saturation(theta * pi, pl);
            const double w = (a.dsig[kk] * pc) / kG;
            const bool cond = s.can && q > s.qs;
            bool wq = cond;
            if (cond) {
                const double C = (q - s.qs) / (1.0 + a.lc * s.dqs);
                q = q - C;
                theta = theta + (a.lc * C) / pi;
                P = P + C * w;
                a.t[o] = (T)theta;
            }
            // (x = 0 also where dt = 0 with tau_e > 0: the formula is then the identity and E = 0, so nothing is lost;
            // a negative dt is taken as given, as the contract's formula takes it)
            if (kk == a.kb && a.x != 0.0) {
                if (cond) s = moist_saturation(theta * pi, pl);      // (the level's updated T)
                const double q_eq = a.rh_s * s.qs;
                if (s.can && q_eq > q) {
                    const double qn = (q + a.x * q_eq) / (1.0 + a.x);
                    E = (qn - q) * w;
                    q = qn;
                    wq = true;
                }
            }
            if (wq) a.q[o] = (T)q;
        }
    }
    if (a.precip && j >= 0 && j < a.H) {
        const long o2 = (long)j * W + i;
        a.precip[o2] = a.precip[o2] + P;
        a.evap[o2] = a.evap[o2] + E;
    }
}

// ---------------------------------------------------------------- the handle's side
// the launches' level tables (pe25d_level_table) and the parameters of the launches that follow
int pe25d_moist_tables(Pe25d *m, const gcm_moist *mo, double dt, std::string *err) {
    if (int rc = moist_check(mo, "moist", err)) return rc;
    if (!std::isfinite(dt)) { *err = "moist: dt must be finite"; return GCM_ERR_ARG; }
    if (!pe25d_level_table(m, "moist", err)) return GCM_ERR_HIP;
    PeMoist &z = m->moist;
    z.kb = (int)(std::max_element(m->sig_host.begin(), m->sig_host.end()) - m->sig_host.begin());
    z.lc = mo->Lv / kCp;
    z.x = mo->tau_e > 0.0 ? dt / mo->tau_e : 0.0;
    z.rh_s = mo->rh_s;
    z.dt = dt;
    return GCM_OK;
}

template <typename T>
static int mo_launch(Pe25d *m, int set, int j0, int j1, int jb0, int jb1, bool accumulate, hipStream_t s, std::string *err) {
    PeBufs<T> &B = bufs<T>(m);
    const PeMoist &z = m->moist;
    MoArgsT<T> a{};
    a.p = B.st[set][GCM_P]; a.t = B.st[set][GCM_T]; a.q = B.st[set][GCM_Q];
    a.sig = m->lev_tab; a.dsig = m->lev_tab + m->L;
    a.exner_tab = m->exner_tab;
    a.precip = accumulate ? z.sums.acc : nullptr;
    a.evap = accumulate ? z.sums.acc + (size_t)m->H * m->W : nullptr;
    a.ptop = m->cfg.ptop; a.lc = z.lc; a.x = z.x; a.rh_s = z.rh_s;
    a.W = m->W; a.L = m->L; a.H = m->H; a.kb = z.kb;
    a.j0 = j0; a.n0 = std::max(0, j1 - j0); a.jb0 = jb0; a.nrows = a.n0 + std::max(0, jb1 - jb0);
    // a launch that accumulates marches whole columns (the column's sum is one register sum in level order); one that
    // does not -- a band's ghost rows -- splits the levels over the grid where the rows alone do not fill the chip, as
    // hs_launch does: every cell's result is independent of the split
    const PhaseColumnGrid g = phase_column_grid(m->W, a.nrows, m->L, m->cus, kMoThreads, !accumulate);
    a.nseg = g.nseg;
    const dim3 grid(g.xb, g.nrows, g.nseg);
    hipLaunchKernelGGL(pe_moist_kernel<T>, grid, dim3(kMoThreads), 0, s, a);
    if (hipGetLastError() != hipSuccess) { *err = "hip: moist kernel launch failed"; return GCM_ERR_HIP; }
    return GCM_OK;
}

// rows [j0, j1) and [jb0, jb1) of state set `set` (-1: the current one) on `s`, pe25d_moist_tables in place.  accumulate:
// the own rows' precipitation and evaporation are added to the registered sums, and the call counts as one application
int pe25d_moist_rows(Pe25d *m, int set, int j0, int j1, int jb0, int jb1, bool keep_ghosts, bool accumulate, hipStream_t s,
                     std::string *err) {
    PeMoist &z = m->moist;
    if (!m->lev_tab) { *err = "moist: no tables in place"; return GCM_ERR_STATE; }
    if (accumulate && !z.sums.acc) { *err = "moist: no sums to accumulate into (gcm_set_moist)"; return GCM_ERR_STATE; }
    if (set < 0) set = m->cur_i;
    if (std::max(0, j1 - j0) + std::max(0, jb1 - jb0) <= 0) return GCM_OK;
    pe25d_phase_wrote(m, set, keep_ghosts, false);         // the launch writes theta and q and reads p, theta and q
    if (int rc = m->f32 ? mo_launch<float>(m, set, j0, j1, jb0, jb1, accumulate, s, err)
                        : mo_launch<double>(m, set, j0, j1, jb0, jb1, accumulate, s, err))
        return rc;
    if (accumulate) sums_count(z.sums, z.dt);
    return GCM_OK;
}

}  // namespace gcm

// GCM_PE25D, Betts-Miller convection (gcm_set_betts_miller, gcm_betts_miller_step): the simplified Betts-Miller scheme of
// Frierson (2007).  Every column relaxes towards the moist adiabat of a parcel lifted from its lowest level and towards a
// fixed relative humidity on it; the precipitation is the water the relaxation removes, and the reference temperature is
// shifted so that the column's enthalpy is conserved.  One launch per step behind the convective adjustment and ahead of
// the moist physics.  The contract: include/gcmcore.h.
//
//   per level k of a column, bottom (k = 0) upwards (float64 for either storage type, rounded once to it):
//     p_lev = sig[k] p + ptop;  Pi = exner(p_lev);  T = theta Pi;  w = (dsig[k] p) / G;  lc = Lv / Cp
//     k = 0:            T_p = T;  q_0 = q[0];  theta_0 = theta[0];  s = moist_saturation(T_p, p_lev)
//     below the LCL:    T_d = theta_0 Pi;  s = moist_saturation(T_d, p_lev);  T_p = T_d
//                       s.q_s <= q_0:  k_lcl = k;  C = (q_0 - s.q_s) / (1 + lc s.dq_s);  T_p = T_d + lc C;
//                                      s = moist_saturation(T_p, p_lev)
//     above k_lcl:      h = (p_lev - p_lev[k-1]) / nsub;  T_c = T_p[k-1];  n = 0 .. nsub - 1:  p_a = p_lev[k-1] + n h
//                         f_1 = slope(T_c, p_a);  T_m = T_c + (0.5 h) f_1;  p_m = p_a + 0.5 h;  f_2 = slope(T_m, p_m)
//                         T_c = T_c + h f_2
//                       T_p = T_c;  s = moist_saturation(T_p, p_lev)
//                       slope(T, p) = (kappa T + (lc q_s) pd) / ((1 + lc dq_s) p),  (q_s, dq_s, pd = p / den) of (T, p)
//     an evaluation that cannot saturate ends the ascent below level k
//     k >= k_lcl:       buoyant = T_p > T (strict; a NaN compares false); buoyant: kt = k; not buoyant with a kt: the
//                       ascent ends below level k
//     the level is taken:  dq = -r (q - rh_bm s.q_s);  dT = -r (T - T_p);  P = P - dq w;  S = S + dT w;  M = M + w
//                          (r = x / (1 + x), x = dt / tau;  P, S, M from 0.0), and P_q, S_T, M_t are P, S, M behind level kt
//   deep convection iff there is a kt and P_q > 0 and S_T > 0:  D = (lc P_q - S_T) / (r M_t);
//     k = 0 .. kt:  theta <- theta + (dT + r D) / Pi;  q <- q + dq;  precip += P_q;  count += 1.  Every other column is
//     not written.
//
// Every operation is rounded on its own: contraction is off for the whole file (the Makefile builds it with
// -ffp-contract=fast-honor-pragmas), host and device, so that a column gets the same bits whichever launch -- a single
// domain's, a band's own rows', a neighbour's ghost rows' -- produces it, and the host probe gcm_betts_miller_columns
// runs the very routines the kernel calls (bm_level, bm_deep, bm_apply).
//
// The state's layout is [j][k][i]: one lane owns the column (j, i), a workgroup is one wave, 64 consecutive i of one
// row, so the request of a level is one contiguous run.
//   pass 1: the column is marched from the bottom, the next level's theta and q requested ahead of the current level's
//     arithmetic (some four exp per level above the LCL, one below it).  A lane leaves the march where its ascent ends.
//     dT and dq of every level taken are parked in LDS, slot-major ([slot][lane]: a wave's access to a slot is 64
//     consecutive words, conflict-free); a runtime-indexed private array would go to scratch.
//   A wave with no deep-convecting lane returns here (__any), having read p, theta and q and written nothing.
//   pass 2, the deep-convecting lanes: levels 0 .. kt again (their lines are still in L2) with the parked changes.
// LDS of a workgroup: the 2 KB Exner table and 16 bytes per level and lane, sized from L at registration: 26 KB at
// L = 24, 160 KB hold L = 158 (kBmMaxLevels).
#pragma clang fp contract(off)
#include <limits>

#include "pe25d_host.h"
#include "pe25d_phase_geometry.h"
#include "pe25d_moist_sat.h"

namespace gcm {

constexpr int kBmThreads = 64;       // one wave: the workgroup's LDS is that wave's parking
constexpr size_t kBmLdsCap = 160 * 1024;   // a workgroup's LDS on gfx950
constexpr size_t kBmSlotBytes = 2 * sizeof(double);   // dT and dq of one level of one lane
constexpr int kBmMaxLevels = (int)((kBmLdsCap - sizeof(double) * kExnerTabDoubles) / (kBmSlotBytes * kBmThreads));
static_assert(kBmMaxLevels == GCM_BETTS_MILLER_MAX_LEVELS, "include/gcmcore.h names the largest L");

// ---------------------------------------------------------------- the column rule (host and device: one set of routines)
struct BmPar { double ptop, lc, r, rh_bm; int nsub; };

// dT and dq of the levels taken: LDS on the device ([slot][lane]), a vector on the host
struct BmLdsPark {
    double *base;                    // + lane
    int L;
    __device__ void put(int k, double dT, double dq) { base[k * kBmThreads] = dT; base[(L + k) * kBmThreads] = dq; }
    __device__ double dT(int k) const { return base[k * kBmThreads]; }
    __device__ double dq(int k) const { return base[(L + k) * kBmThreads]; }
};
struct BmHostPark {
    std::vector<double> v;
    int L;
    explicit BmHostPark(int L_) : v(2 * (size_t)L_), L(L_) {}
    void put(int k, double dT, double dq) { v[k] = dT; v[L + k] = dq; }
    double dT(int k) const { return v[k]; }
    double dq(int k) const { return v[L + k]; }
};

// a column's ascent as far as it got.  The margin fields are the host probe's (MARGIN): the smallest relative distance of
// a comparison consulted, and the sums of |dq w| and |dT w| that P_q and S_T are measured against
struct BmCol {
    double th0 = 0.0, q0 = 0.0;      // the parcel: theta and q of level 0
    double Tp = 0.0, pl = 0.0;       // the parcel at the last level taken: T_p[k - 1], p_lev[k - 1]
    MoistSat sp{0.0, 0.0, 0, 0.0};   // moist_saturation(Tp, pl)
    double P = 0.0, S = 0.0, M = 0.0;       // running over the levels taken
    double Pq = 0.0, ST = 0.0, Mt = 0.0;    // as they stood behind level kt
    int k_lcl = -1, kt = -1;
    bool done = false;
    double margin = std::numeric_limits<double>::infinity(), aP = 0.0, aS = 0.0, aPq = 0.0, aST = 0.0;
};

__host__ __device__ inline double bm_rel(double a, double b) {
    const double m = fmax(fabs(a), fabs(b));
    return m > 0.0 ? fabs(a - b) / m : 0.0;
}

__host__ __device__ inline double bm_slope(const BmPar &b, double T, double p, const MoistSat &s) {
    return (kKappa * T + (b.lc * s.qs) * s.pd) / ((1.0 + b.lc * s.dqs) * p);
}

// level k of the column: theta and q of the level, pc = p of the column.  Sets c.done where the ascent ends below k
template <bool MARGIN, typename Park>
__host__ __device__ inline void bm_level(BmCol &c, const BmPar &b, int k, double theta, double q, double pc, double sigk,
                                         double dsigk, const double *tab, Park &park) {
    const double pl = sigk * pc + b.ptop;
    const double pi = exner(pl, tab);
    const double T = theta * pi;
    double Tp;
    MoistSat s;
    if (k == 0) {
        c.th0 = theta;
        c.q0 = q;
        Tp = T;
        s = moist_saturation(Tp, pl);
        if (!s.can) { c.done = true; return; }
    } else if (c.k_lcl < 0) {
        const double Td = c.th0 * pi;
        s = moist_saturation(Td, pl);
        if (!s.can) { c.done = true; return; }
        Tp = Td;
        if (MARGIN) c.margin = fmin(c.margin, bm_rel(s.qs, c.q0));
        if (s.qs <= c.q0) {
            c.k_lcl = k;
            const double C = (c.q0 - s.qs) / (1.0 + b.lc * s.dqs);
            Tp = Td + b.lc * C;
            s = moist_saturation(Tp, pl);
            if (!s.can) { c.done = true; return; }
        }
    } else {
        const double h = (pl - c.pl) / (double)b.nsub;
        const double hh = 0.5 * h;
        double Tc = c.Tp;
        MoistSat sc = c.sp;
        for (int n = 0; n < b.nsub; ++n) {
            const double pa = c.pl + (double)n * h;
            if (n > 0) {
                sc = moist_saturation(Tc, pa);
                if (!sc.can) { c.done = true; return; }
            }
            const double f1 = bm_slope(b, Tc, pa, sc);
            const double Tm = Tc + hh * f1, pm = pa + hh;
            const MoistSat sm = moist_saturation(Tm, pm);
            if (!sm.can) { c.done = true; return; }
            const double f2 = bm_slope(b, Tm, pm, sm);
            Tc = Tc + h * f2;
        }
        Tp = Tc;
        s = moist_saturation(Tp, pl);
        if (!s.can) { c.done = true; return; }
    }
    bool buoyant = false;
    if (c.k_lcl >= 0) {
        buoyant = Tp > T;
        if (MARGIN) c.margin = fmin(c.margin, bm_rel(Tp, T));
        if (!buoyant && c.kt >= 0) { c.done = true; return; }
    }
    const double w = (dsigk * pc) / kG;
    const double dq = -b.r * (q - b.rh_bm * s.qs);
    const double dT = -b.r * (T - Tp);
    park.put(k, dT, dq);
    c.P = c.P - dq * w;
    c.S = c.S + dT * w;
    c.M = c.M + w;
    if (MARGIN) {
        c.aP = c.aP + fabs(dq * w);
        c.aS = c.aS + fabs(dT * w);
    }
    if (buoyant) {
        c.kt = k;
        c.Pq = c.P; c.ST = c.S; c.Mt = c.M;
        if (MARGIN) { c.aPq = c.aP; c.aST = c.aS; }
    }
    c.Tp = Tp; c.pl = pl; c.sp = s;
}

// behind the march: does the column convect deeply
template <bool MARGIN>
__host__ __device__ inline bool bm_deep(BmCol &c) {
    if (c.kt < 0) return false;
    if (MARGIN) {
        c.margin = fmin(c.margin, c.aPq > 0.0 ? fabs(c.Pq) / c.aPq : 0.0);
        c.margin = fmin(c.margin, c.aST > 0.0 ? fabs(c.ST) / c.aST : 0.0);
    }
    return c.Pq > 0.0 && c.ST > 0.0;
}

// r D of a deep column, and level k <= kt of it
__host__ __device__ inline double bm_shift(const BmCol &c, const BmPar &b) { return b.r * ((b.lc * c.Pq - c.ST) / (b.r * c.Mt)); }
template <typename Park>
__host__ __device__ inline void bm_apply(const BmPar &b, const Park &park, double rD, int k, double pc, double sigk,
                                         const double *tab, double *theta, double *q) {
    const double pi = exner(sigk * pc + b.ptop, tab);
    *theta = *theta + (park.dT(k) + rD) / pi;
    *q = *q + park.dq(k);
}

// ---------------------------------------------------------------- checks and the host probe
int betts_miller_check(const gcm_betts_miller *bm, const char *fn, std::string *err) {
    const auto bad = [&](const char *what) { *err = std::string(fn) + ": " + what; return GCM_ERR_ARG; };
    if (!bm) return bad("no parameters");
    if (!std::isfinite(bm->Lv) || !std::isfinite(bm->tau) || !std::isfinite(bm->rh_bm)) return bad("every parameter must be finite");
    if (!(bm->Lv > 0.0)) return bad("Lv must be > 0");
    if (!(bm->tau > 0.0)) return bad("tau must be > 0");
    if (!(bm->rh_bm > 0.0 && bm->rh_bm <= 1.0)) return bad("rh_bm must lie in (0, 1]");
    if (bm->nsub < 1 || bm->nsub > 8) return bad("nsub must lie in [1, 8]");
    return GCM_OK;
}

static BmPar bm_par(const gcm_betts_miller *bm, double ptop, double dt) {
    const double x = dt / bm->tau;
    return BmPar{ptop, bm->Lv / kCp, x / (1.0 + x), bm->rh_bm, bm->nsub};
}

// gcm_betts_miller_columns: [ncol][L] columns through bm_level / bm_deep / bm_apply; no handle, no device
int betts_miller_columns(int ncol, int L, const double *p, const double *theta, const double *q, const double *sig,
                         const double *dsig, double ptop, double dt, const gcm_betts_miller *bm, double *theta_out,
                         double *q_out, double *precip, int32_t *kt, int32_t *k_lcl, double *margin, std::string *err) {
    if (int rc = betts_miller_check(bm, "gcm_betts_miller_columns", err)) return rc;
    if (ncol < 0 || L < 1 || !std::isfinite(ptop) || !std::isfinite(dt) || (ncol > 0 && (!p || !theta || !q || !sig || !dsig))) {
        *err = "gcm_betts_miller_columns: ncol must be >= 0, L >= 1, ptop and dt finite; p, theta, q, sig and dsig are required";
        return GCM_ERR_ARG;
    }
    double tab[kExnerTabDoubles];
    build_exner_table(tab);
    const BmPar b = bm_par(bm, ptop, dt);
    BmHostPark park(L);
    for (int n = 0; n < ncol; ++n) {
        const size_t o = (size_t)n * L;
        BmCol c;
        for (int k = 0; k < L && !c.done; ++k) bm_level<true>(c, b, k, theta[o + k], q[o + k], p[n], sig[k], dsig[k], tab, park);
        const bool deep = bm_deep<true>(c);
        const double rD = deep ? bm_shift(c, b) : 0.0;
        for (int k = 0; k < L; ++k) {
            double th = theta[o + k], qq = q[o + k];
            if (deep && k <= c.kt) bm_apply(b, park, rD, k, p[n], sig[k], tab, &th, &qq);
            if (theta_out) theta_out[o + k] = th;
            if (q_out) q_out[o + k] = qq;
        }
        if (precip) precip[n] = deep ? c.Pq : 0.0;
        if (kt) kt[n] = deep ? c.kt : -1;
        if (k_lcl) k_lcl[n] = c.k_lcl;
        if (margin) margin[n] = c.margin;
    }
    return GCM_OK;
}

// ---------------------------------------------------------------- the kernel
size_t betts_miller_lds_bytes(int L) { return sizeof(double) * kExnerTabDoubles + kBmSlotBytes * (size_t)L * kBmThreads; }

template <typename T>
struct BmArgsT {
    const T *p;                      // [j][i], interior row 0
    T *t, *q;                        // [j][k][i], interior row 0
    const double *sig, *dsig;        // [L]
    const double *exner_tab;
    double *precip, *count;          // [H][W] own rows, or null: the launch accumulates nothing
    BmPar par;
    int W, L, H;
    int j0, n0, jb0, nrows;          // the rows of the launch: [j0, j0 + n0), then from jb0 on (a band's ghost rows: negative / >= H)
};

// grid (column blocks of 64, rows, 1)
template <typename T>
__global__ __launch_bounds__(kBmThreads) void pe_betts_miller_kernel(BmArgsT<T> a) {
    extern __shared__ double bm_lds[];
    const int W = a.W, L = a.L;
    const int lane = threadIdx.x;
    const int i = blockIdx.x * kBmThreads + lane;
    const int r = (int)blockIdx.y;
    if (r >= a.nrows) return;                              // (uniform: the grid has nrows rows)
    double *tab = bm_lds;
    for (int n = lane; n < kExnerTabDoubles; n += kBmThreads) tab[n] = a.exner_tab[n];
    __syncthreads();
    const int j = r < a.n0 ? a.j0 + r : a.jb0 + (r - a.n0);
    const bool live = i < W;
    const long c3 = (long)j * L * W + (live ? i : 0);      // (a lane past the row loads nothing, stores nothing)
    const double pc = live ? (double)a.p[(long)j * W + i] : 0.0;
    BmLdsPark park{bm_lds + kExnerTabDoubles + lane, L};

    // ---- pass 1: the ascent; level k + 1 is requested ahead of level k's arithmetic
    BmCol c;
    c.done = !live;
    if (live) {
        T th_n = a.t[c3], q_n = a.q[c3];
        for (int k = 0; k < L; ++k) {
            const T th = th_n, qq = q_n;
            if (k + 1 < L) {
                const long o = c3 + (long)(k + 1) * W;
                th_n = a.t[o];
                q_n = a.q[o];
            }
            bm_level<false>(c, a.par, k, (double)th, (double)qq, pc, a.sig[k], a.dsig[k], tab, park);
            if (c.done) break;
        }
    }
    const bool deep = live && bm_deep<false>(c);
    if (!__any(deep ? 1 : 0)) return;
    if (!deep) return;

    // ---- pass 2: the deep-convecting lanes
    const double rD = bm_shift(c, a.par);
    for (int k = 0; k <= c.kt; ++k) {
        const long o = c3 + (long)k * W;
        double theta = (double)a.t[o], q = (double)a.q[o];
        bm_apply(a.par, park, rD, k, pc, a.sig[k], tab, &theta, &q);
        a.t[o] = (T)theta;
        a.q[o] = (T)q;
    }
    if (a.precip && j >= 0 && j < a.H) {
        const long o2 = (long)j * W + i;
        a.precip[o2] = a.precip[o2] + c.Pq;
        a.count[o2] = a.count[o2] + 1.0;
    }
}

// ---------------------------------------------------------------- the handle's side
// What a registration or a step needs of the handle: L >= 2, sig strictly decreasing in k (level 0 is the bottom), and
// the wave's parking at the handle's L within a workgroup's LDS; the kernel's dynamic LDS size is set once, here (the
// kernel is instantiated and launched in this unit alone)
int pe25d_betts_miller_fits(Pe25d *m, const char *fn, std::string *err) {
    PeBettsMiller &z = m->betts_miller;
    if (z.lds_bytes) return GCM_OK;
    if (m->L < 2) { *err = std::string(fn) + ": the scheme needs L >= 2 levels"; return GCM_ERR_UNSUPPORTED; }
    for (int k = 1; k < m->L; ++k)
        if (!(m->sig_host[k] < m->sig_host[k - 1])) {
            *err = std::string(fn) + ": sig must strictly decrease in k (level 0 is the bottom)";
            return GCM_ERR_UNSUPPORTED;
        }
    const size_t need = betts_miller_lds_bytes(m->L);
    if (m->L > kBmMaxLevels || need > kBmLdsCap) {
        *err = std::string(fn) + ": the parked changes of " + std::to_string(m->L) + " levels take " + std::to_string(need) +
               " bytes of LDS, a workgroup has " + std::to_string(kBmLdsCap) + " (L <= " + std::to_string(kBmMaxLevels) + ")";
        return GCM_ERR_UNSUPPORTED;
    }
    const void *k = m->f32 ? (const void *)pe_betts_miller_kernel<float> : (const void *)pe_betts_miller_kernel<double>;
    if (int rc = hip_rc(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need), fn, err)) return rc;
    z.lds_bytes = need;
    return GCM_OK;
}

// the launches' level tables (pe25d_level_table) and the parameters of the launches that follow
int pe25d_betts_miller_tables(Pe25d *m, const gcm_betts_miller *bm, double dt, std::string *err) {
    if (int rc = betts_miller_check(bm, "betts_miller", err)) return rc;
    if (!std::isfinite(dt)) { *err = "betts_miller: dt must be finite"; return GCM_ERR_ARG; }
    if (int rc = pe25d_betts_miller_fits(m, "betts_miller", err)) return rc;
    if (!pe25d_level_table(m, "betts_miller", err)) return GCM_ERR_HIP;
    PeBettsMiller &z = m->betts_miller;
    const BmPar b = bm_par(bm, m->cfg.ptop, dt);
    z.lc = b.lc; z.r = b.r; z.rh_bm = b.rh_bm; z.nsub = b.nsub;
    z.dt = dt;
    return GCM_OK;
}

template <typename T>
static int bm_launch(Pe25d *m, int set, int j0, int j1, int jb0, int jb1, bool accumulate, hipStream_t s, std::string *err) {
    PeBufs<T> &B = bufs<T>(m);
    const PeBettsMiller &z = m->betts_miller;
    BmArgsT<T> a{};
    a.p = B.st[set][GCM_P]; a.t = B.st[set][GCM_T]; a.q = B.st[set][GCM_Q];
    a.sig = m->lev_tab; a.dsig = m->lev_tab + m->L;
    a.exner_tab = m->exner_tab;
    a.precip = accumulate ? z.sums.acc : nullptr;
    a.count = accumulate ? z.sums.acc + (size_t)m->H * m->W : nullptr;
    a.par = BmPar{m->cfg.ptop, z.lc, z.r, z.rh_bm, z.nsub};
    a.W = m->W; a.L = m->L; a.H = m->H;
    a.j0 = j0; a.n0 = std::max(0, j1 - j0); a.jb0 = jb0; a.nrows = a.n0 + std::max(0, jb1 - jb0);
    // every launch marches whole columns: the ascent and its sums run through the levels in order
    const PhaseColumnGrid g = phase_column_grid(m->W, a.nrows, m->L, m->cus, kBmThreads, false);
    const dim3 grid(g.xb, g.nrows, g.nseg);
    hipLaunchKernelGGL(pe_betts_miller_kernel<T>, grid, dim3(kBmThreads), z.lds_bytes, s, a);
    if (hipGetLastError() != hipSuccess) { *err = "hip: betts_miller kernel launch failed"; return GCM_ERR_HIP; }
    return GCM_OK;
}

// rows [j0, j1) and [jb0, jb1) of state set `set` (-1: the current one) on `s`, pe25d_betts_miller_tables in place.
// accumulate: the own rows' precipitation and counts are added to the registered sums, and the call counts as one
// application of dt
int pe25d_betts_miller_rows(Pe25d *m, int set, int j0, int j1, int jb0, int jb1, bool keep_ghosts, bool accumulate,
                            hipStream_t s, std::string *err) {
    PeBettsMiller &z = m->betts_miller;
    if (!m->lev_tab || !z.lds_bytes) { *err = "betts_miller: no tables in place"; return GCM_ERR_STATE; }
    if (accumulate && !z.sums.acc) { *err = "betts_miller: no sums to accumulate into (gcm_set_betts_miller)"; return GCM_ERR_STATE; }
    if (set < 0) set = m->cur_i;
    if (std::max(0, j1 - j0) + std::max(0, jb1 - jb0) <= 0) return GCM_OK;
    pe25d_phase_wrote(m, set, keep_ghosts, false);         // the launch writes theta and q and reads p, theta and q
    if (int rc = m->f32 ? bm_launch<float>(m, set, j0, j1, jb0, jb1, accumulate, s, err)
                        : bm_launch<double>(m, set, j0, j1, jb0, jb1, accumulate, s, err))
        return rc;
    if (accumulate) sums_count(z.sums, z.dt);
    return GCM_OK;
}

}  // namespace gcm

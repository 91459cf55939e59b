// GCM_PE25D, surface fluxes and boundary-layer mixing (gcm_set_boundary_layer, gcm_boundary_layer_step): bulk exchange
// of momentum, heat and moisture with a surface of prescribed temperature and the implicit diffusion that carries it
// upwards, behind the Held-Suarez forcing and ahead of the convective adjustment.  The contract: include/gcmcore.h.
//
//   (A) centre quantities of the column (j, i), i and j periodic, T_s the cell's ground temperature:
//     uc = 0.5 (u[0][j][i] + u[0][j][i-1]);  vc = 0.5 (v[0][j][i] + v[0][j-1][i]);  S = sqrt(uc uc + vc vc)
//     p_s = p + ptop;  p_a = sig[0] p + ptop;  Pi_a = exner(p_a);  T_a = theta[0] Pi_a
//     z_a = ((Rd / G) (T_a (1 + (Rv / Rd - 1) q[0]))) log(p_s / p_a);  cd = cd0 + cd1 min(S, v_cap);  r = S / z_a
//     interfaces m = 0 .. L-2:  sig_e = sig[m] - 0.5 dsig[m];  p_e = sig_e p + ptop
//       T_e = 0.5 (theta[m] Pi_m + theta[m+1] Pi_{m+1});  rho_e = p_e / (Rd T_e);  gr = (G rho_e) / p
//       f = 1 where p_e >= p_pbl, else exp(-(((p_pbl - p_e) / p_strat)^2))
//       e[m] = (((S z_a) f) (gr gr)) / (0.5 (dsig[m] + dsig[m+1]))
//   (B) four column solves, "surface step on level 0, then diffusion", with (x, target, a[m]):
//     theta: (dt ch) r,  T_s / Pi_a,  (dt ce) e[m]          q: (dt ce) r (0 where the surface cannot saturate),  q_ss,  (dt ce) e[m]
//     u: dt (0.5 (cd_i r_i + cd_{i+1} r_{i+1})),  0,  dt (0.5 (cd_i e_i[m] + cd_{i+1} e_{i+1}[m]))        v: likewise in j
//     X0' = (X[0] + x target) / (1 + x)
//     lo[k] = a[k-1] / dsig[k];  up[k] = a[k] / dsig[k]  (a[-1] = a[L-1] = 0);  d = (1 + lo[k]) + up[k]
//     w[0] = 1 / d;  w[k] = 1 / (d - lo[k] g[k-1]);  g[k] = up[k] w[k]
//     y[0] = X0' w[0];  y[k] = (X[k] + lo[k] y[k-1]) w[k];  X[L-1] = y[L-1];  X[k] = y[k] + g[k] X[k+1]
//
// Every operation is float64 and rounded on its own: contraction is off for the whole file (the Makefile builds it with
// -ffp-contract=fast-honor-pragmas), host and device, and the host probes gcm_boundary_layer_surface and
// gcm_boundary_layer_column evaluate the very routines the kernels call (bl_surface, bl_interface, bl_surface_step,
// bl_eliminate, bl_forward; exner() of gcm_math.h is one host and device routine too).
//
// The phase is not column-local: u sits between the centres i and i + 1, v between the rows j and j + 1.  Two launches
// keep it race-free by construction, neither reads a word that another lane of the same launch writes:
//   1. pe_bl_theta_q_kernel: the column's centre quantities from u[0], v[0] (read only), its own theta, q, p and ground
//      temperature; cd, r and e go to float64 scratch fields in the state's layout (e: [j][L-1][i]); theta and q of the
//      own column are solved in the same march, which has theta of two neighbouring levels in hand when it forms e.
//      theta and q share a[m], hence lo, w and g: one elimination serves both;
//   2. pe_bl_wind_kernel: u and v, one grid plane each, from the scratch fields of two neighbouring centre columns and
//      the lane's own column.
// One lane owns a column, a wave is 64 consecutive i of a row and a workgroup of its own: a level's request is one
// contiguous run, levels are requested kBlBatch at a time.  y and g of a solve are parked per lane in LDS, [level][lane]
// (8 bytes a word: no bank conflicts), 1.5 KB a level for theta + q and 1 KB for a wind: 60 KB at L = 40.  Above
// kBlLdsLevels they are parked in float64 scratch fields of the handle instead, with the same arithmetic.  No register
// array is indexed by a loop counter that is not unrolled: the kernels use no scratch memory.
//
// A latitude band that has opted in (gcm_set_band_boundary_layer) takes the BAND form of both kernels over its own rows:
// j does not wrap, rows j - 1 and j + 1 are the neighbouring rows of the band's allocation (ghost rows -1 and H as the
// last exchange and the ghost rows' solar step and Held-Suarez forcing left them).  Launch 1 then runs over rows [0, H]:
// the workgroups of ghost row H form and store cd, r and e only (what v of row H - 1 reads), launch 2 over rows [0, H).
// The arithmetic of a row is the single domain's, in the same order: the same bits.  The ghost rows are not advanced;
// the caller exchanges the edge rows again behind the phase.
#pragma clang fp contract(off)
#include "pe25d_host.h"
#include "pe25d_moist_sat.h"

namespace gcm {

// ---------------------------------------------------------------- the arithmetic (host and device: one set of routines)
struct BlPar { double cd0, cd1, v_cap, p_pbl, p_strat; };
struct BlSurface { double S, z_a, cd, r; };

// (A), the level-0 part; pi_a = exner(sig0 p + ptop)
__host__ __device__ inline BlSurface bl_surface(const BlPar &b, double uc, double vc, double theta0, double q0, double p,
                                                double ptop, double sig0, double pi_a) {
    BlSurface s;
    s.S = sqrt(uc * uc + vc * vc);
    const double p_s = p + ptop;
    const double p_a = sig0 * p + ptop;
    const double T_a = theta0 * pi_a;
    const double Tv = T_a * (1.0 + (kRv / kRd - 1.0) * q0);
    s.z_a = ((kRd / kG) * Tv) * log(p_s / p_a);
    s.cd = b.cd0 + b.cd1 * (s.S < b.v_cap ? s.S : b.v_cap);
    s.r = s.S / s.z_a;
    return s;
}

// (A), e[m] of the interface between levels m and m + 1; Sz = S z_a
__host__ __device__ inline double bl_interface(const BlPar &b, double Sz, double p, double ptop, double sig_m, double dsig_m,
                                               double dsig_m1, double th_m, double pi_m, double th_m1, double pi_m1) {
    const double sig_e = sig_m - 0.5 * dsig_m;
    const double p_e = sig_e * p + ptop;
    const double T_e = 0.5 * (th_m * pi_m + th_m1 * pi_m1);
    const double rho_e = p_e / (kRd * T_e);
    const double gr = (kG * rho_e) / p;
    double f = 1.0;
    if (!(p_e >= b.p_pbl)) {
        const double z = (b.p_pbl - p_e) / b.p_strat;
        f = exp(-(z * z));
    }
    return ((Sz * f) * (gr * gr)) / (0.5 * (dsig_m + dsig_m1));
}

// (B): the surface step, one level of the elimination (a_lo = a[k-1], a_up = a[k]), one level of the forward sweep
__host__ __device__ inline double bl_surface_step(double X0, double x, double target) { return (X0 + x * target) / (1.0 + x); }
struct BlElim { double lo, w, g; };
__host__ __device__ inline BlElim bl_eliminate(int k, double a_lo, double a_up, double dsig_k, double g_prev) {
    BlElim c;
    c.lo = a_lo / dsig_k;
    const double up = a_up / dsig_k;
    const double d = (1.0 + c.lo) + up;
    c.w = k == 0 ? 1.0 / d : 1.0 / (d - c.lo * g_prev);
    c.g = up * c.w;
    return c;
}
__host__ __device__ inline double bl_forward(int k, double X, const BlElim &c, double y_prev) {
    return k == 0 ? X * c.w : (X + c.lo * y_prev) * c.w;
}

int boundary_layer_check(const gcm_boundary_layer *bl, const char *fn, std::string *err) {
    const auto bad = [&](const char *what) { *err = std::string(fn) + ": " + what; return GCM_ERR_ARG; };
    if (!bl) return bad("no parameters");
    for (double v : {bl->cd0, bl->cd1, bl->v_cap, bl->ch, bl->ce, bl->p_pbl, bl->p_strat})
        if (!std::isfinite(v)) return bad("every parameter must be finite");
    if (bl->cd0 < 0.0 || bl->cd1 < 0.0 || bl->ch < 0.0 || bl->ce < 0.0) return bad("cd0, cd1, ch and ce must be >= 0");
    if (!(bl->v_cap > 0.0)) return bad("v_cap must be > 0");
    if (!(bl->p_strat > 0.0)) return bad("p_strat must be > 0");
    return GCM_OK;
}

static BlPar bl_par(const gcm_boundary_layer *bl) { return BlPar{bl->cd0, bl->cd1, bl->v_cap, bl->p_pbl, bl->p_strat}; }

int boundary_layer_surface(int n, const gcm_boundary_layer *bl, double ptop, double sig0, const double *uc, const double *vc,
                           const double *theta0, const double *q0, const double *p, double *S, double *z_a, double *cd,
                           std::string *err) {
    if (int rc = boundary_layer_check(bl, "gcm_boundary_layer_surface", err)) return rc;
    if (n < 0 || (n > 0 && (!uc || !vc || !theta0 || !q0 || !p)) || !std::isfinite(ptop) || !std::isfinite(sig0)) {
        *err = "gcm_boundary_layer_surface: n must be >= 0, ptop and sig0 finite, uc, vc, theta0, q0 and p are required";
        return GCM_ERR_ARG;
    }
    double tab[kExnerTabDoubles];
    build_exner_table(tab);
    const BlPar b = bl_par(bl);
    for (int i = 0; i < n; ++i) {
        const BlSurface s = bl_surface(b, uc[i], vc[i], theta0[i], q0[i], p[i], ptop, sig0, exner(sig0 * p[i] + ptop, tab));
        if (S) S[i] = s.S;
        if (z_a) z_a[i] = s.z_a;
        if (cd) cd[i] = s.cd;
    }
    return GCM_OK;
}

int boundary_layer_column(int ncol, int L, const double *dsig, const double *a, const double *x, const double *target,
                          const double *X, double *X_out, double *X0_surface, std::string *err) {
    if (ncol < 0 || L < 2 || !dsig || (ncol > 0 && (!a || !x || !target || !X || !X_out))) {
        *err = "gcm_boundary_layer_column: ncol must be >= 0, L >= 2, dsig, a, x, target, X and X_out are required";
        return GCM_ERR_ARG;
    }
    std::vector<double> y(L), g(L);
    for (int c = 0; c < ncol; ++c) {
        const double *ac = a + (size_t)c * (L - 1), *Xc = X + (size_t)c * L;
        double *out = X_out + (size_t)c * L;
        const double X0 = bl_surface_step(Xc[0], x[c], target[c]);
        if (X0_surface) X0_surface[c] = X0;
        for (int k = 0; k < L; ++k) {
            const BlElim el = bl_eliminate(k, k > 0 ? ac[k - 1] : 0.0, k < L - 1 ? ac[k] : 0.0, dsig[k], k > 0 ? g[k - 1] : 0.0);
            y[k] = bl_forward(k, k == 0 ? X0 : Xc[k], el, k > 0 ? y[k - 1] : 0.0);
            g[k] = el.g;
        }
        out[L - 1] = y[L - 1];
        for (int k = L - 2; k >= 0; --k) out[k] = y[k] + g[k] * out[k + 1];
    }
    return GCM_OK;
}

// ---------------------------------------------------------------- the kernels
constexpr int kBlLanes = 64;         // a workgroup is one wave: 64 consecutive columns of one row
constexpr int kBlBatch = 4;          // levels requested together, then advanced in order
constexpr int kBlLdsLevels = 40;     // up to here y and g are parked in LDS (60 KB for theta + q), above in scratch fields
// (the largest dynamic request, theta + q at kBlLdsLevels, beside the static Exner table, within a workgroup's default 64 KB)
static_assert(3 * sizeof(double) * kBlLdsLevels * kBlLanes + sizeof(double) * kExnerTabDoubles <= 65536, "theta + q park exceeds 64 KB of LDS");
constexpr int kBlParkFields = 4;     // L > kBlLdsLevels: g, y, y of pe_bl_theta_q_kernel; (g, y) x (u, v) of pe_bl_wind_kernel

template <typename T>
struct BlArgsT {
    const T *p;                      // [j][i]
    T *u, *v, *t, *q;                // [j][k][i]
    const double *gt;                // [j][i]
    const double *sig, *dsig;        // [L]
    const double *exner_tab;
    double *cd, *r, *e;              // scratch: [j][i], [j][i], [j][L-1][i]; a band: H + 1 rows of each
    double *park;                    // L > kBlLdsLevels: kBlParkFields fields [j][L][i] of H rows; else null (LDS)
    double *shf, *evap;              // [H][W], or null: the launch accumulates nothing
    double *sh_j, *evap_kg;          // [j][i], or null: the slab ocean's flux words SH_J and EVAP_KG (pe25d_slab_ocean.hip)
    BlPar par;
    double ptop, dt, dtch, dtce;     // dt ch, dt ce
    int W, H, L;
};

// where a lane parks word `arr` of level k: LDS [arr][k][lane], or the handle's scratch field `arr` at the lane's cell
template <bool LDS>
struct BlPark {
    double *base;
    long field, level;
    __device__ __forceinline__ void put(int arr, int k, double v) const { base[arr * field + k * level] = v; }
    __device__ __forceinline__ double get(int arr, int k) const { return base[arr * field + k * level]; }
};

// grid (tiles of 64 columns, rows); BAND: rows [0, H] of a latitude band, j not periodic, row H forms cd, r and e only
template <typename T, bool LDS, bool BAND>
__global__ __launch_bounds__(kBlLanes) void pe_bl_theta_q_kernel(BlArgsT<T> a) {
    __shared__ double tab[kExnerTabDoubles];
    extern __shared__ double bl_lds[];
    const int lane = (int)threadIdx.x;
    for (int n = lane; n < kExnerTabDoubles; n += kBlLanes) tab[n] = a.exner_tab[n];
    __syncthreads();
    const int W = a.W, H = a.H, L = a.L;
    const int i = (int)blockIdx.x * kBlLanes + lane, j = (int)blockIdx.y;
    if (i >= W || j >= (BAND ? H + 1 : H)) return;
    const long c2 = (long)j * W + i, c3 = (long)j * L * W + i, e3 = (long)j * (L - 1) * W + i;
    const BlPark<LDS> park = LDS ? BlPark<LDS>{bl_lds + lane, (long)L * kBlLanes, kBlLanes}
                                 : BlPark<LDS>{a.park + c3, (long)H * L * W, W};
    const int iw = i == 0 ? W - 1 : i - 1, jn = BAND ? j - 1 : (j == 0 ? H - 1 : j - 1);
    const double pc = (double)a.p[c2], Ts = a.gt[c2];
    const double th0 = (double)a.t[c3], q0 = (double)a.q[c3];
    const double uc = 0.5 * ((double)a.u[c3] + (double)a.u[(long)j * L * W + iw]);
    const double vc = 0.5 * ((double)a.v[c3] + (double)a.v[(long)jn * L * W + i]);
    const double pi_a = exner(a.sig[0] * pc + a.ptop, tab);
    const BlSurface sf = bl_surface(a.par, uc, vc, th0, q0, pc, a.ptop, a.sig[0], pi_a);
    a.cd[c2] = sf.cd;
    a.r[c2] = sf.r;
    const double Sz = sf.S * sf.z_a;
    if (BAND && j == H) {
        // the south ghost row (uniform per workgroup): e of its interfaces from the state as it came in, in the order of
        // the march below; no solve, no store to theta or q, no sum, nothing parked
        double th_c = th0, pi_c = pi_a;
        for (int kk = 0; kk + 1 < L; ++kk) {
            const double th_n = (double)a.t[c3 + (long)(kk + 1) * W];
            const double pi_n = exner(a.sig[kk + 1] * pc + a.ptop, tab);
            a.e[e3 + (long)kk * W] = bl_interface(a.par, Sz, pc, a.ptop, a.sig[kk], a.dsig[kk], a.dsig[kk + 1], th_c, pi_c, th_n, pi_n);
            th_c = th_n; pi_c = pi_n;
        }
        return;
    }
    const MoistSat ss = moist_saturation(Ts, pc + a.ptop);
    const double th0n = bl_surface_step(th0, a.dtch * sf.r, Ts / pi_a);
    const double q0n = bl_surface_step(q0, ss.can ? a.dtce * sf.r : 0.0, ss.qs);
    if (a.shf) {
        const double mass = (a.dsig[0] * pc) / kG;
        a.shf[c2] = a.shf[c2] + ((kCp * pi_a) * (th0n - th0)) * mass;
        a.evap[c2] = a.evap[c2] + (q0n - q0) * mass;
    }
    if (a.sh_j) {
        // the slab ocean is registered: the step's own increments of shf and evap, the same expressions, J / m^2 and kg / m^2
        const double mass = (a.dsig[0] * pc) / kG;
        a.sh_j[c2] = ((kCp * pi_a) * (th0n - th0)) * mass;
        a.evap_kg[c2] = (q0n - q0) * mass;
    }
    // the march up: level kk with theta of level kk + 1 in hand (e of the interface above it, from the state at entry)
    double th_c = th0, pi_c = pi_a;                      // level kk as it came in
    double Xt = th0n, Xq = q0n;                          // level kk as the solve takes it
    double a_prev = 0.0, g_prev = 0.0, yt = 0.0, yq = 0.0;
    for (int k = 0; k < L; k += kBlBatch) {
        T tn[kBlBatch], qn[kBlBatch];                    // levels k + 1 .. k + kBlBatch
#pragma unroll
        for (int n = 0; n < kBlBatch; ++n) {
            const int kn = k + 1 + n;
            if (kn >= L) break;
            tn[n] = a.t[c3 + (long)kn * W];
            qn[n] = a.q[c3 + (long)kn * W];
        }
#pragma unroll
        for (int n = 0; n < kBlBatch; ++n) {
            const int kk = k + n;
            if (kk >= L) break;
            double a_k = 0.0, th_n = 0.0, q_n = 0.0, pi_n = 0.0;
            if (kk + 1 < L) {
                th_n = (double)tn[n];
                q_n = (double)qn[n];
                pi_n = exner(a.sig[kk + 1] * pc + a.ptop, tab);
                const double e = bl_interface(a.par, Sz, pc, a.ptop, a.sig[kk], a.dsig[kk], a.dsig[kk + 1], th_c, pi_c, th_n, pi_n);
                a.e[e3 + (long)kk * W] = e;
                a_k = a.dtce * e;
            }
            const BlElim el = bl_eliminate(kk, a_prev, a_k, a.dsig[kk], g_prev);
            yt = bl_forward(kk, Xt, el, yt);
            yq = bl_forward(kk, Xq, el, yq);
            park.put(0, kk, el.g);
            park.put(1, kk, yt);
            park.put(2, kk, yq);
            a_prev = a_k; g_prev = el.g;
            th_c = th_n; pi_c = pi_n; Xt = th_n; Xq = q_n;
        }
    }
    // the march down
    double xt = yt, xq = yq;
    a.t[c3 + (long)(L - 1) * W] = (T)xt;
    a.q[c3 + (long)(L - 1) * W] = (T)xq;
    for (int k = L - 2; k >= 0; --k) {
        const double g = park.get(0, k);
        xt = park.get(1, k) + g * xt;
        xq = park.get(2, k) + g * xq;
        a.t[c3 + (long)k * W] = (T)xt;
        a.q[c3 + (long)k * W] = (T)xq;
    }
}

// grid (tiles of 64 columns, rows, 2): plane 0 solves u (between the centres i and i + 1), plane 1 v (rows j and j + 1);
// BAND: rows [0, H) of a latitude band, row j + 1 of the scratch fields does not wrap (row H: the south ghost row's)
template <typename T, bool LDS, bool BAND>
__global__ __launch_bounds__(kBlLanes) void pe_bl_wind_kernel(BlArgsT<T> a) {
    extern __shared__ double bl_lds[];
    const int lane = (int)threadIdx.x;
    const int W = a.W, H = a.H, L = a.L;
    const int i = (int)blockIdx.x * kBlLanes + lane, j = (int)blockIdx.y, f = (int)blockIdx.z;
    if (i >= W || j >= H) return;
    const long c2 = (long)j * W + i, c3 = (long)j * L * W + i;
    const int i2 = f == 0 ? (i + 1 == W ? 0 : i + 1) : i, j2 = f == 0 ? j : (!BAND && j + 1 == H ? 0 : j + 1);
    const long n2 = (long)j2 * W + i2;
    const long ea = (long)j * (L - 1) * W + i, eb = (long)j2 * (L - 1) * W + i2;
    const BlPark<LDS> park = LDS ? BlPark<LDS>{bl_lds + lane, (long)L * kBlLanes, kBlLanes}
                                 : BlPark<LDS>{a.park + (long)(2 * f) * H * L * W + c3, (long)H * L * W, W};
    T *const X = f == 0 ? a.u : a.v;
    const double cd_a = a.cd[c2], cd_b = a.cd[n2];
    const double x = a.dt * (0.5 * (cd_a * a.r[c2] + cd_b * a.r[n2]));
    double a_prev = 0.0, g_prev = 0.0, y = 0.0;
    for (int k = 0; k < L; k += kBlBatch) {
        T xn[kBlBatch];
        double e_a[kBlBatch], e_b[kBlBatch];
#pragma unroll
        for (int n = 0; n < kBlBatch; ++n) {
            const int kk = k + n;
            if (kk >= L) break;
            xn[n] = X[c3 + (long)kk * W];
            if (kk + 1 < L) {
                e_a[n] = a.e[ea + (long)kk * W];
                e_b[n] = a.e[eb + (long)kk * W];
            }
        }
#pragma unroll
        for (int n = 0; n < kBlBatch; ++n) {
            const int kk = k + n;
            if (kk >= L) break;
            const double a_k = kk + 1 < L ? a.dt * (0.5 * (cd_a * e_a[n] + cd_b * e_b[n])) : 0.0;
            const double Xk = kk == 0 ? bl_surface_step((double)xn[n], x, 0.0) : (double)xn[n];
            const BlElim el = bl_eliminate(kk, a_prev, a_k, a.dsig[kk], g_prev);
            y = bl_forward(kk, Xk, el, y);
            park.put(0, kk, el.g);
            park.put(1, kk, y);
            a_prev = a_k; g_prev = el.g;
        }
    }
    double xv = y;
    X[c3 + (long)(L - 1) * W] = (T)xv;
    for (int k = L - 2; k >= 0; --k) {
        xv = park.get(1, k) + park.get(0, k) * xv;
        X[c3 + (long)k * W] = (T)xv;
    }
}

// ---------------------------------------------------------------- the handle's side
// rows of cd, r and e: a band's own rows and its first south ghost row (what v of row H - 1 reads)
static size_t bl_centre_rows(const Pe25d *m) { return (size_t)m->H + (m->wrap ? 0 : 1); }
static size_t bl_scratch_words(const Pe25d *m) {
    const size_t cells = (size_t)m->H * m->W, centres = bl_centre_rows(m) * m->W;
    return centres * (2 + (size_t)(m->L - 1)) + (m->L > kBlLdsLevels ? cells * m->L * kBlParkFields : 0);
}

// what a registration or a step needs of the handle.  GCM_ERR_UNSUPPORTED: a latitude band that has not opted in (the
// centre quantities of the outer ghost rows need rows that do not exist: the phase takes the own rows and the caller
// exchanges the edge rows again, gcm_set_band_boundary_layer), L < 2, levels that do not start at the bottom;
// GCM_ERR_STATE: no ground
int pe25d_boundary_layer_fits(Pe25d *m, const char *fn, std::string *err) {
    const auto no = [&](int rc, const char *what) { *err = std::string(fn) + ": " + what; return rc; };
    if (!m->wrap && !m->boundary.band)
        return no(GCM_ERR_UNSUPPORTED, "single domains only (a latitude band's ghost rows cannot be advanced locally: gcm_set_band_boundary_layer)");
    if (m->L < 2) return no(GCM_ERR_UNSUPPORTED, "L must be 2 or more");
    for (int k = 1; k < m->L; ++k)
        if (!(m->sig_host[k] < m->sig_host[k - 1])) return no(GCM_ERR_UNSUPPORTED, "sig must decrease strictly with k (level 0 is the bottom)");
    if (!m->gt_set) return no(GCM_ERR_STATE, "set the ground temperature first (gcm_set_ground)");
    return GCM_OK;
}

// gcm_set_band_boundary_layer: a band takes the phase over its own rows and three exchanges per step
int pe25d_set_band_boundary_layer(Pe25d *m, bool on, std::string *err) {
    if (m->wrap) {
        if (!on) return GCM_OK;
        *err = "gcm_set_band_boundary_layer: GCM_PE25D latitude bands only (a single domain takes gcm_set_boundary_layer directly)";
        return GCM_ERR_UNSUPPORTED;
    }
    if (!on && m->boundary.sums.acc) {
        *err = "gcm_set_band_boundary_layer: the boundary layer is registered (gcm_set_boundary_layer(NULL) first)";
        return GCM_ERR_STATE;
    }
    m->boundary.band = on;
    return GCM_OK;
}
bool pe25d_band_boundary_layer(const Pe25d *m) { return !m->wrap && m->boundary.band; }

// the scratch fields: in place (on; allocated by the first call), or freed
int pe25d_boundary_layer_scratch(Pe25d *m, bool on, hipStream_t s, std::string *err) {
    PeBoundary &z = m->boundary;
    if (on) {
        if (z.scratch) return GCM_OK;
        if (!dev_upload<double>(m, &z.scratch, nullptr, bl_scratch_words(m))) { *err = "hip: boundary layer scratch allocation failed"; return GCM_ERR_HIP; }
        return GCM_OK;
    }
    if (!z.scratch) return GCM_OK;
    if (int rc = hip_rc(hipStreamSynchronize(s), "gcm_set_boundary_layer", err)) return rc;   // (a launch may still use them)
    m->allocs.erase(std::remove(m->allocs.begin(), m->allocs.end(), (void *)z.scratch), m->allocs.end());
    (void)hipFree(z.scratch);
    z.scratch = nullptr;
    return GCM_OK;
}

// the level tables and the scratch fields in place, and (bl, dt) as the parameters of the launches that follow
int pe25d_boundary_layer_tables(Pe25d *m, const gcm_boundary_layer *bl, double dt, hipStream_t s, std::string *err) {
    if (int rc = boundary_layer_check(bl, "boundary layer", err)) return rc;
    if (!std::isfinite(dt)) { *err = "boundary layer: dt must be finite"; return GCM_ERR_ARG; }
    if (int rc = pe25d_boundary_layer_fits(m, "boundary layer", err)) return rc;
    if (!pe25d_level_table(m, "boundary layer", err)) return GCM_ERR_HIP;
    if (int rc = pe25d_boundary_layer_scratch(m, true, s, err)) return rc;
    m->boundary.par = *bl;
    m->boundary.dt = dt;
    return GCM_OK;
}

template <typename T, bool BAND>
static int bl_launch(Pe25d *m, int set, bool accumulate, hipStream_t s, std::string *err) {
    PeBufs<T> &B = bufs<T>(m);
    const PeBoundary &z = m->boundary;
    const size_t cells = (size_t)m->H * m->W, centres = bl_centre_rows(m) * m->W;
    BlArgsT<T> a{};
    a.p = B.st[set][GCM_P]; a.u = B.st[set][GCM_U]; a.v = B.st[set][GCM_V]; a.t = B.st[set][GCM_T]; a.q = B.st[set][GCM_Q];
    a.gt = m->gt;
    a.sig = m->lev_tab; a.dsig = m->lev_tab + m->L;
    a.exner_tab = m->exner_tab;
    a.cd = z.scratch; a.r = a.cd + centres; a.e = a.r + centres;
    const bool lds = m->L <= kBlLdsLevels;
    a.park = lds ? nullptr : a.e + centres * (size_t)(m->L - 1);
    a.shf = accumulate ? z.sums.acc : nullptr;
    a.evap = accumulate ? z.sums.acc + cells : nullptr;
    a.sh_j = pe25d_slab_ocean_word(m, GCM_SLAB_SH_J);     // (null without the slab ocean)
    a.evap_kg = pe25d_slab_ocean_word(m, GCM_SLAB_EVAP_KG);
    a.par = bl_par(&z.par);
    a.ptop = m->cfg.ptop; a.dt = z.dt; a.dtch = z.dt * z.par.ch; a.dtce = z.dt * z.par.ce;
    a.W = m->W; a.H = m->H; a.L = m->L;
    const unsigned tiles = (unsigned)((m->W + kBlLanes - 1) / kBlLanes);
    const size_t word = sizeof(double) * (size_t)m->L * kBlLanes;
    const unsigned rows1 = (unsigned)bl_centre_rows(m);
    if (lds) hipLaunchKernelGGL((pe_bl_theta_q_kernel<T, true, BAND>), dim3(tiles, rows1), dim3(kBlLanes), 3 * word, s, a);
    else hipLaunchKernelGGL((pe_bl_theta_q_kernel<T, false, BAND>), dim3(tiles, rows1), dim3(kBlLanes), 0, s, a);
    if (hipGetLastError() != hipSuccess) { *err = "hip: boundary layer theta / q kernel launch failed"; return GCM_ERR_HIP; }
    if (lds) hipLaunchKernelGGL((pe_bl_wind_kernel<T, true, BAND>), dim3(tiles, m->H, 2), dim3(kBlLanes), 2 * word, s, a);
    else hipLaunchKernelGGL((pe_bl_wind_kernel<T, false, BAND>), dim3(tiles, m->H, 2), dim3(kBlLanes), 0, s, a);
    if (hipGetLastError() != hipSuccess) { *err = "hip: boundary layer wind kernel launch failed"; return GCM_ERR_HIP; }
    return GCM_OK;
}

// every row of state set `set` (-1: the current one) of a single domain, or the own rows of a band that has opted in
// (its ghost rows -1 and H must be current, and those of u, v, theta and q are stale behind the call until the edge rows
// are exchanged again), on `s`, pe25d_boundary_layer_tables in place.
// accumulate: the heat and the water the surface gave go to the registered sums, and the call counts as one application
int pe25d_boundary_layer_rows(Pe25d *m, int set, bool keep_ghosts, bool accumulate, hipStream_t s, std::string *err) {
    PeBoundary &z = m->boundary;
    if (!m->lev_tab || !z.scratch) { *err = "boundary layer: no tables in place"; return GCM_ERR_STATE; }
    if (accumulate && !z.sums.acc) { *err = "boundary layer: no sums to accumulate into (gcm_set_boundary_layer)"; return GCM_ERR_STATE; }
    if (set < 0) set = m->cur_i;
    pe25d_phase_wrote(m, set, keep_ghosts, true);          // the launches write u, v, theta and q
    if (int rc = m->wrap ? (m->f32 ? bl_launch<float, false>(m, set, accumulate, s, err) : bl_launch<double, false>(m, set, accumulate, s, err))
                         : (m->f32 ? bl_launch<float, true>(m, set, accumulate, s, err) : bl_launch<double, true>(m, set, accumulate, s, err)))
        return rc;
    if (accumulate) sums_count(z.sums, z.dt);
    return GCM_OK;
}

}  // namespace gcm

// GCM_PE25D, the Held & Suarez (1994) forcing (gcm_set_held_suarez, gcm_held_suarez_step): Newtonian relaxation of theta
// towards a prescribed equilibrium and Rayleigh friction of the low-level winds, backward Euler, one launch per step
// behind the corrector (and behind the solar step where gcm_set_physics is on).  The contract: include/gcmcore.h.
//
//   tables (host, float64; gcm_held_suarez_tables):
//     r[k]  = max(0, (sig[k] - sigma_b) / (1 - sigma_b));   fu[k] = 1 / (1 + (dt k_f) r[k])
//     c2[j] = cos(lat[j])^2;   s2[j] = sin(lat[j])^2;      kt[k][j] = k_a + (((k_s - k_a) r[k]) c2[j]) c2[j]
//   update (device, float64 for either storage type, rounded once to it):
//     r[k] > 0:  u <- u fu[k],  v <- v fu[k]
//     p_lev = sig[k] p + ptop;  theta_eq = max(T_min (P0 / p_lev)^kappa, T_0 - dT_y s2[j] - (dtheta_z ln(p_lev / P0)) c2[j])
//     theta <- (theta + (dt kt) theta_eq) * (1 / (1 + dt kt))          (dt kt and the reciprocal: host tables)
//
// Every operation is rounded on its own: contraction is off for the whole file (the Makefile builds it with
// -ffp-contract=fast-honor-pragmas), host and device, so that the host tables are the NumPy restatement's bits and a
// cell gets the same bits whichever launch -- a single domain's, a band's own rows', a neighbour's ghost rows', any
// split of the levels -- produces it.
//
// The state's layout is [j][k][i]: one lane owns the column (j, i) and marches a segment of its levels, a wave is 64
// consecutive i of one row, so the request of a level is one contiguous run.  p is read once per column and segment,
// theta read and written once, u and v read and written on the friction levels only; the level and latitude tables
// are wave-uniform.  No LDS but the 2 KB Exner table.
#pragma clang fp contract(off)
#include "pe25d_host.h"
#include "pe25d_phase_geometry.h"

namespace gcm {

// ---------------------------------------------------------------- the tables (host)
int held_suarez_check(const gcm_held_suarez *hs, const char *fn, std::string *err) {
    const auto bad = [&](const char *what) { *err = std::string(fn) + ": " + what; return GCM_ERR_ARG; };
    if (!hs) return bad("no parameters");
    const double v[8] = {hs->k_f, hs->k_a, hs->k_s, hs->sigma_b, hs->dT_y, hs->dtheta_z, hs->T_0, hs->T_min};
    for (const double x : v)
        if (!std::isfinite(x)) return bad("every parameter must be finite");
    if (hs->k_f < 0.0 || hs->k_a < 0.0 || hs->k_s < 0.0) return bad("k_f, k_a and k_s must be >= 0");
    if (!(hs->sigma_b >= 0.0 && hs->sigma_b < 1.0)) return bad("sigma_b must lie in [0, 1)");
    if (!hs->lat) return bad("the lat table is required");
    return GCM_OK;
}

static double hs_r(double sig, double sigma_b) {
    const double num = sig - sigma_b;
    const double den = 1.0 - sigma_b;
    return std::max(0.0, num / den);
}

int held_suarez_tables(int L, const double *sig, int nlat, const double *lat, const gcm_held_suarez *hs, double dt,
                       double *fu, double *kt, double *s2, double *c2, std::string *err) {
    const char *fn = "gcm_held_suarez_tables";
    const auto bad = [&](const char *what) { *err = std::string(fn) + ": " + what; return GCM_ERR_ARG; };
    if (L < 1 || nlat < 1) return bad("L and nlat must be 1 or more");
    if (!sig || !fu || !kt || !s2 || !c2) return bad("a null pointer");
    gcm_held_suarez p{};
    if (hs) p = *hs;
    if (hs && !p.lat) p.lat = lat;                          // (the table's latitudes are the argument's)
    if (int rc = held_suarez_check(hs ? &p : nullptr, fn, err)) return rc;
    if (!lat) return bad("the lat table is required");
    if (!std::isfinite(dt)) return bad("dt must be finite");
    for (int k = 0; k < L; ++k)
        if (!std::isfinite(sig[k])) return bad("sig must be finite");
    for (int j = 0; j < nlat; ++j)
        if (!std::isfinite(lat[j])) return bad("lat must be finite");
    for (int j = 0; j < nlat; ++j) {
        const double c = std::cos(lat[j]), s = std::sin(lat[j]);
        c2[j] = c * c;
        s2[j] = s * s;
    }
    const double dk = dt * p.k_f;
    const double ks_a = p.k_s - p.k_a;
    for (int k = 0; k < L; ++k) {
        const double r = hs_r(sig[k], p.sigma_b);
        const double d = dk * r;
        fu[k] = 1.0 / (1.0 + d);
        const double kr = ks_a * r;
        for (int j = 0; j < nlat; ++j) {
            const double a = kr * c2[j];
            const double b = a * c2[j];
            kt[(size_t)k * nlat + j] = p.k_a + b;
        }
    }
    return GCM_OK;
}

// ---------------------------------------------------------------- the kernel
// (kHsThreads, kHsBatch -- levels requested together, then advanced in order: pe25d_phase_geometry.h)
template <typename T>
struct HsArgsT {
    const T *p;                      // [j][i], interior row 0
    T *t, *u, *v;                    // [j][k][i], interior row 0
    const double *fric;              // [L] fu[k] where r[k] > 0, else -1: the level's winds are not touched
    const double *sig;               // [L]
    const double *sigmk, *lnsig;     // [L] sig^-kappa, ln(sig) (FACT)
    const double *s2, *c2;           // [Hg]
    const double *adt, *binv;        // [L][Hg] dt kt, 1 / (1 + dt kt)
    const double *exner_tab;
    double ptop, T_min, T_0, dT_y, dtheta_z;
    int W, L, Hg, row0;
    int j0, n0, jb0, nrows;          // the rows of the launch: [j0, j0 + n0), then from jb0 on (a band's ghost rows: negative / >= H)
    int nseg;                        // gridDim.z: segment s marches levels [s L / nseg, (s + 1) L / nseg)
};

// grid (column blocks, rows, level segments).  FACT (ptop == 0, the reference's geometry), as pe_radiation_kernel's:
// (P0 / p_lev)^kappa = (P0 / p)^kappa sig^-kappa and ln(p_lev / P0) = ln(p / P0) + ln(sig) -- one Exner evaluation and one
// logarithm per column and segment instead of one per cell; the level parts come from the host in extended precision.
template <typename T, bool FACT>
__global__ __launch_bounds__(kHsThreads) void pe_held_suarez_kernel(HsArgsT<T> a) {
    __shared__ double tab[kExnerTabDoubles];
    for (int n = threadIdx.x; n < kExnerTabDoubles; n += kHsThreads) tab[n] = a.exner_tab[n];
    __syncthreads();
    const int W = a.W, L = a.L;
    const int i = blockIdx.x * kHsThreads + threadIdx.x;
    const int r = (int)blockIdx.y;
    if (i >= W || r >= a.nrows) return;
    const int j = r < a.n0 ? a.j0 + r : a.jb0 + (r - a.n0);
    const int jg = wrapi(a.row0 + j, a.Hg);
    const int seg = (int)blockIdx.z;
    const int k0 = (int)((long)seg * L / a.nseg), k1 = (int)((long)(seg + 1) * L / a.nseg);
    const long c3 = (long)j * L * W + i;
    const double pc = (double)a.p[(long)j * W + i];
    const double c2 = a.c2[jg];
    const double t_surf = a.T_0 - a.dT_y * a.s2[jg];
    double pk_col = 0.0, ln_col = 0.0;
    if (FACT) {
        pk_col = rcp(exner(pc, tab));                       // (P0 / p)^kappa
        ln_col = log(pc / kP0);
    }
    for (int k = k0; k < k1; k += kHsBatch) {
        T th[kHsBatch], uu[kHsBatch], vv[kHsBatch];
        double f[kHsBatch];
#pragma unroll
        for (int n = 0; n < kHsBatch; ++n) {
            const int kk = k + n;
            if (kk >= k1) break;
            const long o = c3 + (long)kk * W;
            th[n] = a.t[o];
            f[n] = a.fric[kk];
            if (f[n] > 0.0) { uu[n] = a.u[o]; vv[n] = a.v[o]; }
        }
#pragma unroll
        for (int n = 0; n < kHsBatch; ++n) {
            const int kk = k + n;
            if (kk >= k1) break;
            const long o = c3 + (long)kk * W;
            double pk, ln;
            if (FACT) {
                pk = pk_col * a.sigmk[kk];
                ln = ln_col + a.lnsig[kk];
            } else {
                const double pl = a.sig[kk] * pc + a.ptop;
                pk = rcp(exner(pl, tab));
                ln = log(pl / kP0);
            }
            const double cold = a.T_min * pk;
            const double warm = t_surf - (a.dtheta_z * ln) * c2;
            const double th_eq = fmax(cold, warm);
            const double adt = a.adt[(long)kk * a.Hg + jg], binv = a.binv[(long)kk * a.Hg + jg];
            a.t[o] = (T)(((double)th[n] + adt * th_eq) * binv);
            if (f[n] > 0.0) {
                a.u[o] = (T)((double)uu[n] * f[n]);
                a.v[o] = (T)((double)vv[n] * f[n]);
            }
        }
    }
}

// ---------------------------------------------------------------- the tables' way to the device
// layout of PeHeldSuarez::tab (doubles): fric, sig, sigmk, lnsig [L] | s2, c2 [Hg] | adt, binv [L][Hg]
static size_t hs_tab_doubles(const Pe25d *m) { return (size_t)4 * m->L + (size_t)2 * m->Hg + (size_t)2 * m->L * m->Hg; }

int pe25d_hs_tables(Pe25d *m, const gcm_held_suarez *hs, double dt, hipStream_t s, std::string *err) {
    if (int rc = held_suarez_check(hs, "held_suarez", err)) return rc;
    const int L = m->L, Hg = m->Hg;
    std::vector<double> key = {hs->k_f, hs->k_a, hs->k_s, hs->sigma_b, hs->dT_y, hs->dtheta_z, hs->T_0, hs->T_min, dt};
    key.insert(key.end(), hs->lat, hs->lat + Hg);
    PeHeldSuarez &z = m->hs;
    if (z.tab && z.key.size() == key.size() && !memcmp(z.key.data(), key.data(), sizeof(double) * key.size())) return GCM_OK;
    std::vector<double> T(hs_tab_doubles(m)), fu(L), kt((size_t)L * Hg);
    double *fric = T.data(), *sig = fric + L, *sigmk = sig + L, *lnsig = sigmk + L, *s2 = lnsig + L, *c2 = s2 + Hg,
           *adt = c2 + Hg, *binv = adt + (size_t)L * Hg;
    if (int rc = held_suarez_tables(L, m->sig_host.data(), Hg, hs->lat, hs, dt, fu.data(), kt.data(), s2, c2, err)) return rc;
    for (int k = 0; k < L; ++k) {
        const double sg = m->sig_host[k];
        fric[k] = hs_r(sg, hs->sigma_b) > 0.0 ? fu[k] : -1.0;
        sig[k] = sg;
        sigmk[k] = (double)powl((long double)sg, -(long double)kKappa);
        lnsig[k] = (double)logl((long double)sg);
        for (int j = 0; j < Hg; ++j) {
            const double x = dt * kt[(size_t)k * Hg + j];
            adt[(size_t)k * Hg + j] = x;
            binv[(size_t)k * Hg + j] = 1.0 / (1.0 + x);
        }
    }
    // A change is rare (another dt, another registration): everything queued so far -- it may still read the tables in
    // place, on the caller's stream or, a band, on the second stream -- ends first, and the upload is synchronous
    if (hipStreamSynchronize(s) != hipSuccess || (m->aux && hipStreamSynchronize(m->aux) != hipSuccess)) {
        *err = "hip: held_suarez: the launches ahead of the table upload failed"; return GCM_ERR_HIP;
    }
    if (!z.tab && !dev_upload<double>(m, &z.tab, nullptr, T.size())) { *err = "hip: held_suarez table allocation failed"; return GCM_ERR_HIP; }
    if (hipMemcpy(z.tab, T.data(), sizeof(double) * T.size(), hipMemcpyHostToDevice) != hipSuccess) {
        z.key.clear();
        *err = "hip: held_suarez table upload failed"; return GCM_ERR_HIP;
    }
    z.key.swap(key);
    z.par[0] = hs->T_min; z.par[1] = hs->T_0; z.par[2] = hs->dT_y; z.par[3] = hs->dtheta_z;
    return GCM_OK;
}

// ---------------------------------------------------------------- the launch
template <typename T>
static int hs_launch(Pe25d *m, int set, int j0, int j1, int jb0, int jb1, hipStream_t s, std::string *err) {
    PeBufs<T> &B = bufs<T>(m);
    const int L = m->L, Hg = m->Hg;
    HsArgsT<T> a{};
    a.p = B.st[set][GCM_P]; a.t = B.st[set][GCM_T]; a.u = B.st[set][GCM_U]; a.v = B.st[set][GCM_V];
    a.fric = m->hs.tab; a.sig = a.fric + L; a.sigmk = a.sig + L; a.lnsig = a.sigmk + L;
    a.s2 = a.lnsig + L; a.c2 = a.s2 + Hg; a.adt = a.c2 + Hg; a.binv = a.adt + (size_t)L * Hg;
    a.exner_tab = m->exner_tab;
    a.ptop = m->cfg.ptop; a.T_min = m->hs.par[0]; a.T_0 = m->hs.par[1]; a.dT_y = m->hs.par[2]; a.dtheta_z = m->hs.par[3];
    a.W = m->W; a.L = L; a.Hg = Hg; a.row0 = m->cfg.row0;
    a.j0 = j0; a.n0 = std::max(0, j1 - j0); a.jb0 = jb0; a.nrows = a.n0 + std::max(0, jb1 - jb0);
    // the levels are split over the grid where the rows alone do not fill the chip (a band's ghost rows, a small band)
    const PhaseColumnGrid g = phase_column_grid(m->W, a.nrows, L, m->cus, kHsThreads, true);
    a.nseg = g.nseg;
    const dim3 grid(g.xb, g.nrows, g.nseg);
    if (m->cfg.ptop == 0.0) hipLaunchKernelGGL((pe_held_suarez_kernel<T, true>), grid, dim3(kHsThreads), 0, s, a);
    else hipLaunchKernelGGL((pe_held_suarez_kernel<T, false>), grid, dim3(kHsThreads), 0, s, a);
    if (hipGetLastError() != hipSuccess) { *err = "hip: held_suarez kernel launch failed"; return GCM_ERR_HIP; }
    return GCM_OK;
}

int pe25d_hs_rows(Pe25d *m, int set, int j0, int j1, int jb0, int jb1, bool keep_ghosts, hipStream_t s, std::string *err) {
    if (!m->hs.tab || m->hs.key.empty()) { *err = "held_suarez: no tables in place"; return GCM_ERR_STATE; }
    if (set < 0) set = m->cur_i;
    if (std::max(0, j1 - j0) + std::max(0, jb1 - jb0) <= 0) return GCM_OK;
    const bool own = std::max(j0, 0) < std::min(j1, m->H) || std::max(jb0, 0) < std::min(jb1, m->H);
    // a band's own edge rows, marched in level segments, get their column sums on the third stream right behind the edge
    // rows' pack (update_edges): that launch reads the u and v this one is about to write
    if (own && m->aux2 && m->edge_cs_set == set) {
        (void)hipStreamWaitEvent(s, m->ev_cs, 0);
        m->edge_cs_set = -1;
    }
    pe25d_phase_wrote(m, set, keep_ghosts, true);          // the launch writes theta, u and v and reads p with them
    return m->f32 ? hs_launch<float>(m, set, j0, j1, jb0, jb1, s, err) : hs_launch<double>(m, set, j0, j1, jb0, jb1, s, err);
}

}  // namespace gcm

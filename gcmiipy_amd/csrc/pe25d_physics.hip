// GCM_PE25D column physics: grey radiation (gcm_grey_radiation, gcm_solar_step, a band's rows through gcm_set_physics)
// and the ground temperature it advances.  The kernel, its level and lat / lon tables and its launches live here and
// nowhere else; the handle: pe25d_host.h.
#include "pe25d_host.h"

namespace gcm {

// ---------------------------------------------------------------- grey radiation (column physics)
// basic_grey_radiation (grey_solar.py:358-563) + solar_timestep (no_limits_2_5d.py:66-75):
// one thread per (j,i) column, the upwelling scan bottom-up, the downwelling scan top-down.
template <typename T>
struct RadArgsT {
    const double *tlw, *tsw, *csw_top, *clw_b_div, *swfac;   // [L] level tables (host-built)
    const double *sigk;                                      // [L] sig^kappa (FACT, see pe_radiation_kernel)
    const double *sig, *dsig;                                // [L] the handle's float64 level table (pe25d_level_table)
    const double *coslat, *sinlat, *lon;                     // [Hg], [Hg], [W]
    double *gt;                                              // ground temperature [H][W]
    T *dTdt, *dtg;                                           // tendencies out of the diagnostic form (3-D, 2-D scratch)
    double hour_angle, albedo, dt;
    int apply;                                               // 1: t, gt updated in place
    int j0, n0, jb0;                                         // rows of the launch: [j0, j0 + n0), then from jb0 on (a band's ghost
                                                             // rows on either side in one launch: negative / >= H)
    // BUDGET only (the slab ocean is registered, pe25d_slab_ocean.hip): the flux words SC, SW_SFC, LW_DOWN, LW_UP, OLR,
    // `bud_stride` words apart, at interior row 0; tcol: the long-wave transmissivity of the whole column
    double *bud;
    long bud_stride;
    double tcol;
};

// The arithmetic is float64 for either storage type T, and so is every table the kernel reads -- the level tables
// below and sig / dsig, which come from the handle's float64 level table, not from the T copies the dynamics use: the
// column physics is a small share of a step, and the fp32 variant then differs from fp64 only by the rounding of what
// it stores (p, theta, and the diagnostic form's dTdt and dt_ground; the ground temperature is float64 on either).
// One thread per column.  The long-wave absorption needs the upwelling flux from BELOW a level and
// the downwelling flux from ABOVE it, two opposite scans: the bottom-up scan parks one value per
// level (the absorbed upwelling) and the top-down scan recomputes the level's emission from theta
// (LMAX > 0: kept in registers from the one up-front request of the column; LMAX == 0: read again).
// LMAX > 0: L <= LMAX and the parked column lives in registers (loops unrolled); LMAX == 0: any L,
// parked in LDS, park[L][threads].  The kernel reads theta and writes it (apply) or dTdt (diagnostic);
// nothing else goes through HBM.
// FACT (ptop == 0, the reference's geometry): the Exner factor of level k is (p sig_k / P0)^kappa =
// (p / P0)^kappa sig_k^kappa -- ONE table-and-series evaluation per column and a product per use instead of
// three evaluations per level (emission in either scan, to_potential_temp); sig^kappa comes from the host in
// extended precision.  The product differs from the direct evaluation by an ulp or two of a factor that enters
// theta -> T -> theta symmetrically, far inside the 1e-10 of the parity tests (golden g13, the 2880x1440x40 strips).
// BUDGET (launched only while the slab ocean is registered, always in place): the ground temperature is left to the slab
// (pe_slab_ocean_kernel); in place of its update the lane stores the column's five flux words in W / m^2 -- SC = Sc,
// SW_SFC = S, LW_DOWN = B, LW_UP = U_s and OLR = up + U_s tcol, `up` the bottom-up scan's value above the last level.
// theta takes the very statements of the other instantiations, which the flag does not touch: they compile to the code
// they compiled to without it.
constexpr int kRadTabs = 7;      // per level: tlw, clw_b_div, swfac, sig, dsig, sig^kappa, (free)
template <typename T, int LMAX, bool FACT = false, bool BUDGET = false>
__global__ __launch_bounds__(kRadThreads) void pe_radiation_kernel(PeArgsT<T> a, RadArgsT<T> r, T *t_inout) {
    __shared__ double tab[kExnerTabDoubles];
    __shared__ double lev[kRadTabs][LMAX > 0 ? LMAX : 1];
    extern __shared__ unsigned char rad_park_raw[];
    for (int n = threadIdx.x; n < kExnerTabDoubles; n += kRadThreads) tab[n] = a.exner_tab[n];
    const int W = a.W, L = a.L;
    if (LMAX > 0) {
        // the level tables go to LDS (read from global memory inside the scans, every one of their
        // waits would also wait for the theta column still in flight)
        for (int k = threadIdx.x; k < LMAX; k += kRadThreads) {
            const int kk = min(k, L - 1);
            lev[0][k] = r.tlw[kk]; lev[1][k] = r.clw_b_div[kk]; lev[2][k] = r.swfac[kk];
            lev[3][k] = r.sig[kk]; lev[4][k] = r.dsig[kk];
            if (FACT) lev[5][k] = r.sigk[kk];
        }
    }
    __syncthreads();
    constexpr double kSolar = 1.3608 * 1000.0, kSb = 5.67e-8, kCg = 1.13e6;   // constants.py:59,71,25
    double *p_lwb = (double *)rad_park_raw + threadIdx.x;
    double lwb_reg[LMAX > 0 ? LMAX : 1];
    const int i = blockIdx.x * kRadThreads + threadIdx.x;
    const int j = (int)blockIdx.y < r.n0 ? r.j0 + (int)blockIdx.y : r.jb0 + ((int)blockIdx.y - r.n0);
    if (i >= W) return;
    const int jg = wrapi(a.row0 + j, a.Hg);
    const long c3 = (long)j * L * W + i, c2 = (long)j * W + i;
    // LMAX > 0: the whole theta column is requested before any of it is used (one memory latency per
    // column instead of one per level and scan) and kept: the top-down scan does not read it again
    T tcol[LMAX > 0 ? LMAX : 1];
    if (LMAX > 0) {
#pragma unroll
        for (int k = 0; k < LMAX; ++k) tcol[k] = t_inout[c3 + (long)min(k, L - 1) * W];
    }
    const double pc = (double)a.p[c2], gt = r.gt[c2], ptop = (double)a.ptop;
    // zenith_angle, grey_solar.py:49-65 (declination 0)
    const double pa = r.lon[i] + r.hour_angle;
    const double sza = fmax(r.sinlat[jg] * 0.0 + r.coslat[jg] * 1.0 * cos(pa), 0.0);
    const double Sc = kSolar * sza;
    const double S = (1 - r.albedo) * Sc * r.csw_top[0];
    const double g2 = gt * gt;
    const double U_s = 1 * kSb * (g2 * g2);
    const auto tlw = [&](int k) { return LMAX > 0 ? lev[0][k] : r.tlw[k]; };
    const auto clw = [&](int k) { return LMAX > 0 ? lev[1][k] : r.clw_b_div[k]; };
    const auto swf = [&](int k) { return LMAX > 0 ? lev[2][k] : r.swfac[k]; };
    const auto sig = [&](int k) { return LMAX > 0 ? lev[3][k] : r.sig[k]; };
    const auto dsg = [&](int k) { return LMAX > 0 ? lev[4][k] : r.dsig[k]; };
    const double ex_col = FACT ? exner(pc, tab) : 0.0;
    const auto exk = [&](int k) { return FACT ? ex_col * lev[5][LMAX > 0 ? k : 0] : exner(pc * sig(k) + ptop, tab); };
    // true temperature and emission of one level (to_true_temp; grey_solar.py emission)
    const auto emission = [&](int k, double *tt_out) {
        const double th = LMAX > 0 ? (double)tcol[LMAX > 0 ? k : 0] : (double)t_inout[c3 + (long)k * W];
        const double tt = th * exk(k);
        const double t2 = tt * tt;
        *tt_out = tt;
        return (1 - tlw(k)) * kSb * (t2 * t2);
    };
    double B = 0.0, up = 0.0;
    constexpr int kUnroll = LMAX > 0 ? LMAX : 2;
#pragma unroll kUnroll
    for (int k = 0; k < (LMAX > 0 ? LMAX : L); ++k) {       // bottom-up: emission, B, LWA_b
        if (LMAX > 0 && k >= L) break;
        double tt;
        const double em = emission(k, &tt);
        B += em * clw(k);
        const double lwb = up * (1 - tlw(k));
        if (LMAX > 0) lwb_reg[k] = lwb;
        else p_lwb[k * kRadThreads] = lwb;
        up = up * tlw(k) + em;
    }
    const double dtg = (B + S - U_s) / kCg / (.1);
    if (BUDGET) {
        r.bud[c2] = Sc;
        r.bud[c2 + r.bud_stride] = S;
        r.bud[c2 + 2 * r.bud_stride] = B;
        r.bud[c2 + 3 * r.bud_stride] = U_s;
        r.bud[c2 + 4 * r.bud_stride] = up + U_s * r.tcol;
    } else if (r.apply) r.gt[c2] = gt + dtg * r.dt;
    else r.dtg[c2] = (T)dtg;
    double down = 0.0;
#pragma unroll kUnroll
    for (int kk = 0; kk < (LMAX > 0 ? LMAX : L); ++kk) {     // top-down: LWA_a, then eq. 2.34
        const int k = (LMAX > 0 ? LMAX : L) - 1 - kk;
        if (LMAX > 0 && k >= L) continue;
        const long o = c3 + (long)k * W;
        double tt;
        const double em = emission(k, &tt);
        const double lwa = down * (1 - tlw(k));
        down = down * tlw(k) + em;
        const double U_n = clw(k) * U_s * (1 - tlw(k));
        const double S_n = swf(k) * Sc;
        const double lwb = LMAX > 0 ? lwb_reg[k] : p_lwb[k * kRadThreads];
        const double dTdt = (U_n + S_n - 2 * em + lwa + lwb) * (kG / (kCp * pc * dsg(k)));
        if (r.apply) {
            const double tt_n = tt + dTdt * r.dt;
            t_inout[o] = (T)(tt_n * rcp(exk(k)));                  // to_potential_temp
        } else {
            r.dTdt[o] = (T)dTdt;
        }
    }
}

// pe25d_create: the dynamic LDS size of the LDS-parked form
bool radiation_lds_attribute(const Pe25d *m) {
    const int bytes = (int)(sizeof(double) * (size_t)m->L * kRadThreads);
    if (hipFuncSetAttribute(m->f32 ? (const void *)pe_radiation_kernel<float, 0> : (const void *)pe_radiation_kernel<double, 0>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
    return hipFuncSetAttribute(m->f32 ? (const void *)pe_radiation_kernel<float, 0, false, true> : (const void *)pe_radiation_kernel<double, 0, false, true>,
                               hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess;
}

int pe25d_ground(Pe25d *m, bool set, const double *in, double *out, hipStream_t s, std::string *err) {
    const size_t bytes = sizeof(double) * (size_t)m->H * m->W;
    hipError_t e = set ? hipMemcpyAsync(m->gt, in, bytes, hipMemcpyHostToDevice, s)
                       : hipMemcpyAsync(out, m->gt, bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { *err = "hip: ground temperature transfer failed"; return GCM_ERR_HIP; }
    if (set) {
        m->gt_set = true;
        m->k4_fork_valid = false;
    }
    return GCM_OK;
}

// the one place that picks the instantiation: by L, the GENERIC switch and ptop, with or without BUDGET
template <typename T, bool BUDGET>
static void radiation_dispatch(const Pe25d *m, const dim3 &gg, const PeArgsT<T> &a, const RadArgsT<T> &r, T *th, hipStream_t s) {
    const int L = m->L;
    const bool generic = m->rad_generic;
    const bool fact = m->cfg.ptop == 0.0 && r.sigk != nullptr;
    if (L <= 24 && !generic && fact) hipLaunchKernelGGL((pe_radiation_kernel<T, 24, true, BUDGET>), gg, dim3(kRadThreads), 0, s, a, r, th);
    else if (L <= 40 && !generic && fact) hipLaunchKernelGGL((pe_radiation_kernel<T, 40, true, BUDGET>), gg, dim3(kRadThreads), 0, s, a, r, th);
    else if (L <= 24 && !generic) hipLaunchKernelGGL((pe_radiation_kernel<T, 24, false, BUDGET>), gg, dim3(kRadThreads), 0, s, a, r, th);
    else if (L <= 40 && !generic) hipLaunchKernelGGL((pe_radiation_kernel<T, 40, false, BUDGET>), gg, dim3(kRadThreads), 0, s, a, r, th);
    else hipLaunchKernelGGL((pe_radiation_kernel<T, 0, false, BUDGET>), gg, dim3(kRadThreads), sizeof(double) * (size_t)L * kRadThreads, s, a, r, th);
}

// rows [j0, j1) and [jb0, jb1) of state set `set` (a band's ghost rows: negative, or >= H); keep_ghosts: the caller
// radiates the ghost rows itself before their column sums and anchors are queued (gcm_band_run), so what
// pe25d_prep_ghost_rows left stays valid
// budget: the in-place launch of a step while the slab ocean is registered (pe25d_solar_rows): the BUDGET instantiation
template <typename T>
static int radiation_launch(Pe25d *m, int set, int j0, int j1, int jb0, int jb1, bool keep_ghosts, bool apply, double dt,
                            double hour_angle, double albedo, double *dTdt_host, double *dtg_host, hipStream_t s,
                            std::string *err, bool budget = false) {
    PeBufs<T> &B = bufs<T>(m);
    const int W = m->W, L = m->L, Hg = m->Hg;
    const int nrows = std::max(0, j1 - j0) + std::max(0, jb1 - jb0);
    if (nrows <= 0) return GCM_OK;
    PeArgsT<T> a = make_args<T>(m, set, set, dt);
    a.p = B.st[set][GCM_P];                               // (make_args takes the base state from the current set)
    RadArgsT<T> r{};
    r.j0 = j0; r.n0 = std::max(0, j1 - j0); r.jb0 = jb0;
    r.tlw = m->rad_tab; r.tsw = r.tlw + L; r.csw_top = r.tsw + L; r.clw_b_div = r.csw_top + L; r.swfac = r.clw_b_div + L;
    r.sigk = r.swfac + L;
    r.sig = m->lev_tab; r.dsig = m->lev_tab + L;
    r.coslat = m->rad_geo; r.sinlat = m->rad_geo + Hg; r.lon = m->rad_geo + 2 * Hg;
    r.gt = m->gt;
    r.dTdt = B.pgfu; r.dtg = B.pit;
    r.hour_angle = hour_angle;
    r.albedo = albedo; r.dt = dt; r.apply = apply ? 1 : 0;
    if (apply && !keep_ghosts) m->ghost_ready = -1;        // theta changes in place
    m->last_stage_set = -1;                                // gcm_get_intermediate: theta changed, or pgfu / pit hold the tendencies
    // the diagnostic form writes pgfu / pit on `s`, and a band's explicit solar_timestep changes the ghost rows' theta
    // there: the next stage's chain B (K1 + pit, the ghost rows' anchors) follows the stream's position, not just the last K4
    if (!(apply && (keep_ghosts || m->wrap))) m->k4_fork_valid = false;
    {
        const dim3 gg((W + kRadThreads - 1) / kRadThreads, nrows);
        T *th = B.st[set][GCM_T];
        if (budget && apply) {
            // the column's transmissivity: tcol = clw_b_div[L-1] * tlw[L-1], formed here, once a launch, from the host copy
            // of the tables in place (clw_b_div[L-1] is the product of tlw[0 .. L-2] in the order of grey_radiation_tables)
            r.bud = pe25d_slab_ocean_word(m, GCM_SLAB_SC);
            r.bud_stride = (long)rows_alloc(m) * W;
            r.tcol = m->rad_tab_host[(size_t)3 * L + L - 1] * m->rad_tab_host[(size_t)L - 1];
            if (!r.bud) { *err = "radiation: no slab ocean registered for the budget launch"; return GCM_ERR_STATE; }
            radiation_dispatch<T, true>(m, gg, a, r, th, s);
        } else {
            radiation_dispatch<T, false>(m, gg, a, r, th, s);
        }
    }
    if (hipGetLastError() != hipSuccess) { *err = "hip: radiation kernel launch failed"; return GCM_ERR_HIP; }
    // solar_timestep (apply) stays asynchronous on `s`; the diagnostics form copies its results back
    if (dtg_host && field_to_host(m, dtg_host, B.pit, 1, s) != hipSuccess) { *err = "hip: dt_ground copy-back failed"; return GCM_ERR_HIP; }
    if (dTdt_host && field_to_host(m, dTdt_host, B.pgfu, L, s) != hipSuccess) { *err = "hip: dTdt copy-back failed"; return GCM_ERR_HIP; }
    if ((dtg_host || dTdt_host) && hipStreamSynchronize(s) != hipSuccess) {
        *err = "hip: radiation kernel failed"; return GCM_ERR_HIP;
    }
    return GCM_OK;
}

// gcm_grey_radiation, gcm_solar_step, gcm_set_physics and gcm_grey_radiation_tables: the parameters the radiation
// accepts.  t_lw and t_sw, the transmissivities of the whole column, lie in (0, 1]; albedo in [0, 1].  dsig (may be
// null: not checked): no level's transmissivity t^dsig[k] may round to 0 -- the level tables divide by it (t_lw = 0:
// clw_b_div = 0 / 0, as in the reference's own formula; t_lw = 1e-300: 1 - (1 - t^dsig) = 0 in every level)
int grey_check(int L, const double *dsig, double t_lw, double t_sw, double albedo, const char *fn, std::string *err) {
    const auto bad = [&](const char *what) { *err = std::string(fn) + ": " + what; return GCM_ERR_ARG; };
    if (!(t_lw > 0.0 && t_lw <= 1.0)) return bad("t_lw must lie in (0, 1]");
    if (!(t_sw > 0.0 && t_sw <= 1.0)) return bad("t_sw must lie in (0, 1]");
    if (!(albedo >= 0.0 && albedo <= 1.0)) return bad("albedo must lie in [0, 1]");
    for (int k = 0; dsig && k < L; ++k) {
        if (!(dsig[k] > 0.0) || !std::isfinite(dsig[k])) return bad("dsig must be positive and finite");
        if (!(1 - (1 - std::pow(t_lw, dsig[k])) > 0.0)) return bad("t_lw is too small: a level's long-wave transmissivity rounds to 0");
        if (!(1 - (1 - std::pow(t_sw, dsig[k])) > 0.0)) return bad("t_sw is too small: a level's short-wave transmissivity rounds to 0");
    }
    return GCM_OK;
}

// grey_check on the handle's own levels
int pe25d_grey_check(const Pe25d *m, double t_lw, double t_sw, double albedo, const char *fn, std::string *err) {
    return grey_check(m->L, m->dsig_host.data(), t_lw, t_sw, albedo, fn, err);
}

// The level tables of the radiation kernel for (t_lw, t_sw), out[6][L]: tlw, tsw, csw_top, clw_b_div, swfac, sig^kappa --
// what pe25d_physics_tables uploads and what gcm_grey_radiation_tables returns (no handle, no device).  Same expression
// order as grey_solar.py:323-333,377-385,541; sig^kappa in extended precision (FACT)
int grey_radiation_tables(int L, const double *dsig, const double *sig, double t_lw, double t_sw, double *out, std::string *err) {
    const char *fn = "gcm_grey_radiation_tables";
    const auto bad = [&](const char *what) { *err = std::string(fn) + ": " + what; return GCM_ERR_ARG; };
    if (L < 1) return bad("L must be 1 or more");
    if (!dsig || !sig || !out) return bad("a null pointer");
    if (int rc = grey_check(L, dsig, t_lw, t_sw, 0.0, fn, err)) return rc;
    for (int k = 0; k < L; ++k)
        if (!(sig[k] > 0.0) || !std::isfinite(sig[k])) return bad("sig must be positive and finite");
    double *tlw = out, *tsw = tlw + L, *csw = tsw + L, *cdiv = csw + L, *swf = cdiv + L;
    for (int k = 0; k < L; ++k) {
        tlw[k] = 1 - (1 - std::pow(t_lw, dsig[k]));
        tsw[k] = 1 - (1 - std::pow(t_sw, dsig[k]));
    }
    double c = 1.0;
    for (int k = L - 1; k >= 0; --k) { c = k == L - 1 ? tsw[k] : c * tsw[k]; csw[k] = c; }
    for (int k = 0; k < L; ++k) { c = k == 0 ? tlw[k] : c * tlw[k]; cdiv[k] = c / tlw[k]; }
    for (int k = 0; k < L; ++k) swf[k] = (1 - tsw[k]) * csw[k] / tsw[k];
    for (int k = 0; k < L; ++k) swf[L + k] = (double)powl((long double)sig[k], (long double)kKappa);   // sig^kappa (FACT)
    return GCM_OK;
}

// the level tables (t_lw, t_sw) and the lat / lon tables of the radiation kernel, uploaded when they change
int pe25d_physics_tables(Pe25d *m, double t_lw, double t_sw, const double *lat, const double *lon, hipStream_t s,
                         std::string *err) {
    if (!m->gt_set) { *err = "radiation: set the ground temperature first (gcm_set_ground)"; return GCM_ERR_STATE; }
    if (!lat || !lon) { *err = "radiation: lat and lon tables are required"; return GCM_ERR_ARG; }
    const int W = m->W, L = m->L, Hg = m->Hg;
    if (!pe25d_level_table(m, "radiation", err)) return GCM_ERR_HIP;      // sig and dsig in float64, for either storage type
    bool uploaded = false;
    if (m->rad_key[0] != t_lw || m->rad_key[1] != t_sw || !m->rad_tab) {
        // the tables are built aside: a refused pair leaves the ones in place, and their key, as they were
        std::vector<double> fresh((size_t)6 * L, 0.0);
        if (int rc = grey_radiation_tables(L, m->dsig_host.data(), m->sig_host.data(), t_lw, t_sw, fresh.data(), err)) return rc;
        if (!m->rad_tab && !dev_upload<double>(m, &m->rad_tab, nullptr, (size_t)6 * L)) {
            *err = "hip: radiation table allocation failed"; return GCM_ERR_HIP;
        }
        // the host copy lives in the handle until the next change, so the asynchronous upload may
        // read it after this call returns; a change waits for the previous upload first
        if (hipStreamSynchronize(s) != hipSuccess) { *err = "hip: radiation table upload failed"; return GCM_ERR_HIP; }
        m->rad_tab_host.swap(fresh);
        if (hipMemcpyAsync(m->rad_tab, m->rad_tab_host.data(), sizeof(double) * 6 * L, hipMemcpyHostToDevice, s) != hipSuccess) {
            *err = "hip: radiation table upload failed"; return GCM_ERR_HIP;
        }
        m->rad_key[0] = t_lw; m->rad_key[1] = t_sw;
        uploaded = true;
    }
    // lat / lon tables: uploaded when their content changes (normally once)
    if (m->rad_latlon.size() != (size_t)Hg + W || memcmp(m->rad_latlon.data(), lat, sizeof(double) * Hg) ||
        memcmp(m->rad_latlon.data() + Hg, lon, sizeof(double) * W)) {
        if (hipStreamSynchronize(s) != hipSuccess) { *err = "hip: radiation geometry upload failed"; return GCM_ERR_HIP; }
        m->rad_latlon.assign(lat, lat + Hg);
        m->rad_latlon.insert(m->rad_latlon.end(), lon, lon + W);
        std::vector<double> &Gt = m->rad_geo_host;
        Gt.assign((size_t)2 * Hg + W, 0.0);
        for (int j = 0; j < Hg; ++j) { Gt[j] = std::cos(lat[j]); Gt[Hg + j] = std::sin(lat[j]); }
        for (int i = 0; i < W; ++i) Gt[2 * Hg + i] = lon[i];
        if (!m->rad_geo && !dev_upload<double>(m, &m->rad_geo, nullptr, Gt.size())) {
            *err = "hip: radiation geometry allocation failed"; return GCM_ERR_HIP;
        }
        if (hipMemcpyAsync(m->rad_geo, Gt.data(), sizeof(double) * Gt.size(), hipMemcpyHostToDevice, s) != hipSuccess) {
            *err = "hip: radiation geometry upload failed"; return GCM_ERR_HIP;
        }
        uploaded = true;
    }
    // (a band radiates its ghost rows on the second stream: the tables are in place before anything is queued there)
    if (uploaded && hipStreamSynchronize(s) != hipSuccess) { *err = "hip: radiation table upload failed"; return GCM_ERR_HIP; }
    return GCM_OK;
}

// solar_timestep (no_limits_2_5d.py:66-75) of rows [j0, j1) and [jb0, jb1) of state set `set` (-1: the current one) on stream `s`;
// the tables must be in place (pe25d_physics_tables)
int pe25d_solar_rows(Pe25d *m, int set, int j0, int j1, int jb0, int jb1, bool keep_ghosts, double dt, double utc, double albedo,
                     hipStream_t s, std::string *err) {
    // gcm_set_gas_radiation: the registered gas radiation takes the solar step's place (pe25d_gas_radiation.hip)
    if (pe25d_gas_radiation_on(m)) return pe25d_gas_radiation_rows(m, set, j0, j1, jb0, jb1, keep_ghosts, dt, utc, s, err);
    if (set < 0) set = m->cur_i;
    const double hour_angle = utc / (-24 * 3600.0) * 360 * (M_PI / 180);      // grey_solar.py:51
    const bool budget = m->slab.on;                        // the slab ocean advances the ground temperature
    return m->f32 ? radiation_launch<float>(m, set, j0, j1, jb0, jb1, keep_ghosts, true, dt, hour_angle, albedo, nullptr, nullptr, s, err, budget)
                  : radiation_launch<double>(m, set, j0, j1, jb0, jb1, keep_ghosts, true, dt, hour_angle, albedo, nullptr, nullptr, s, err, budget);
}

// basic_grey_radiation (+ optional in-place solar_timestep).  dTdt_host / dtg_host may be null.  On a latitude
// band the in-place form advances the ghost rows too (their theta as the post-corrector exchange delivered it,
// their ground temperature as the last message delivered it): the neighbour's own inputs, the neighbour's own bits.
int pe25d_radiation(Pe25d *m, bool apply, double dt, double utc, double t_lw, double t_sw, double albedo,
                    const double *lat, const double *lon, double *dTdt_host, double *dtg_host,
                    hipStream_t s, std::string *err) {
    int rc = pe25d_physics_tables(m, t_lw, t_sw, lat, lon, s, err);
    if (rc) return rc;
    const double hour_angle = utc / (-24 * 3600.0) * 360 * (M_PI / 180);      // grey_solar.py:51
    const int g = (apply && !m->wrap) ? kGhost : 0;
    return m->f32 ? radiation_launch<float>(m, m->cur_i, -g, m->H + g, 0, 0, false, apply, dt, hour_angle, albedo, dTdt_host, dtg_host, s, err)
                  : radiation_launch<double>(m, m->cur_i, -g, m->H + g, 0, 0, false, apply, dt, hour_angle, albedo, dTdt_host, dtg_host, s, err);
}

}  // namespace gcm

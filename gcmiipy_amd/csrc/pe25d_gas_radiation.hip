// GCM_PE25D, grey radiation that absorbs by water vapour and CO2 (gcm_set_gas_radiation, gcm_gas_radiation,
// gcm_gas_radiation_step): the reference's grey_radiation (grey_solar.py:192-320) with clouds off, as a phase that takes
// the solar step's place while it is registered.  The contract: include/gcmcore.h; the column routine: pe25d_gas_radiation.h.
//
// Every operation is float64 for either storage type and rounded on its own: contraction is off for the whole file (the
// Makefile builds it with -ffp-contract=fast-honor-pragmas), host and device, and the host probe
// gcm_gas_radiation_columns evaluates the very routine the kernel calls.
//
// pe_gas_radiation_kernel: one lane per column, a workgroup is one wave of 64 consecutive columns of one row, grid (tiles
// of 64 columns, rows), the last tile ragged.  One form for every L: the bottom-up scan parks the long wave a level
// absorbed from below in LDS, park[L][64], and the top-down scan forms the level's powers and emission again instead of
// parking them too (profiles/gas_radiation/README.md says why).  No register array, hence no scratch at any L.
// theta and q are read where a scan uses them, twice each; theta is written (in place) or dt_air (diagnostic).
// BUDGET (launched only while the slab ocean is registered, always in place): the ground temperature is left to the slab
// and the lane stores the column's five flux words, as pe_radiation_kernel's BUDGET instantiations do.
#pragma clang fp contract(off)
#include "pe25d_host.h"
#include "pe25d_gas_radiation.h"

namespace gcm {

constexpr int kGasLanes = 64;
constexpr int kGasMaxL = 120;                                // park[L][64] and the Exner table within 64 KiB of LDS

template <typename T>
struct GasArgsT {
    const T *p, *q;                                          // [j][i], [j][k][i], interior row 0
    T *t;                                                    // theta [j][k][i]: read, and written in place (apply)
    const double *exner_tab;
    const double *sig, *dsig;                                // [L] the handle's float64 level table
    const double *coslat, *sinlat, *lon;                     // [Hg], [Hg], [W]
    const double *sc_row;                                    // [Hg] insolation per global row ("uniform", "daily")
    double *gt;                                              // ground temperature [j][i]
    T *dt_air;                                               // diagnostic form: [j][k][i]
    double *dtg, *olr;                                       // diagnostic form: [H][W] each
    double *bud;                                             // BUDGET: the flux words SC .. OLR, `bud_stride` apart
    long bud_stride;
    GasPar par;
    double S0, sin_d, cos_d, hour_angle, dt, ptop;
    int zenith, apply;
    int W, L, Hg, row0;
    int j0, n0, jb0;                                         // rows of the launch: [j0, j0 + n0), then from jb0 on
};

template <typename T, bool BUDGET>
__global__ __launch_bounds__(kGasLanes) void pe_gas_radiation_kernel(GasArgsT<T> a) {
    __shared__ double tab[kExnerTabDoubles];
    extern __shared__ double gas_park[];
    for (int n = threadIdx.x; n < kExnerTabDoubles; n += kGasLanes) tab[n] = a.exner_tab[n];
    __syncthreads();
    const int W = a.W, L = a.L;
    const int i = (int)blockIdx.x * kGasLanes + (int)threadIdx.x;
    const int j = (int)blockIdx.y < a.n0 ? a.j0 + (int)blockIdx.y : a.jb0 + ((int)blockIdx.y - a.n0);
    if (i >= W) return;
    const int jg = wrapi(a.row0 + j, a.Hg);
    const long c3 = (long)j * L * W + i, c2 = (long)j * W + i;
    const double pc = (double)a.p[c2], gt = a.gt[c2];
    const double SC = a.zenith ? a.S0 * gas_cos_zenith(a.sinlat[jg], a.coslat[jg], a.sin_d, a.cos_d, a.lon[i] + a.hour_angle)
                               : a.sc_row[jg];
    double *const park = gas_park + threadIdx.x;
    const GasColumn c = gas_column(
        L, a.par, SC, gt,
        [&](int k) {
            const long o = c3 + (long)k * W;
            GasLevelIn in;
            in.tp = pc * a.sig[k] + a.ptop;
            in.dp = pc * a.dsig[k];
            in.ex = exner(in.tp, tab);
            in.tt = (double)a.t[o] * in.ex;                  // to_true_temp
            in.q = (double)a.q[o];
            return in;
        },
        [&](int k) -> double & { return park[k * kGasLanes]; },
        [&](int k, double dt_air, const GasLevelIn &in) {
            const long o = c3 + (long)k * W;
            if (a.apply) {
                const double tt_n = in.tt + dt_air * a.dt;   // solar_timestep
                a.t[o] = (T)(tt_n / in.ex);                  // to_potential_temp
            } else {
                a.dt_air[o] = (T)dt_air;
            }
        });
    if (BUDGET) {
        a.bud[c2] = SC;
        a.bud[c2 + a.bud_stride] = c.sw_sfc;
        a.bud[c2 + 2 * a.bud_stride] = c.lw_down;
        a.bud[c2 + 3 * a.bud_stride] = c.lw_up;
        a.bud[c2 + 4 * a.bud_stride] = c.olr;
    } else if (a.apply) {
        a.gt[c2] = gt + c.dt_ground * a.dt;
    } else {
        a.dtg[c2] = c.dt_ground;
        a.olr[c2] = c.olr;
    }
}

// ---------------------------------------------------------------- parameters, the insolation table and the host probe
int gas_radiation_check(const gcm_gas_radiation_par *g, const char *fn, std::string *err) {
    const auto bad = [&](const char *what) { *err = std::string(fn) + ": " + what; return GCM_ERR_ARG; };
    if (!g) return bad("no parameters");
    const double w[6] = {g->k_h2o_lw, g->k_co2_lw, g->k_h2o_sw, g->k_co2_sw, g->co2_vmr, g->solar_constant};
    for (double x : w)
        if (!std::isfinite(x) || x < 0.0) return bad("the weights, co2_vmr and solar_constant must be finite and >= 0");
    if (!(g->ground_albedo >= 0.0 && g->ground_albedo < 1.0)) return bad("ground_albedo must lie in [0, 1)");
    if (!(std::fabs(g->declination) <= M_PI / 2)) return bad("declination must lie in [-pi/2, pi/2]");
    if (g->insolation != GCM_INSOLATION_UNIFORM && g->insolation != GCM_INSOLATION_ZENITH && g->insolation != GCM_INSOLATION_DAILY)
        return bad("unknown insolation");
    return GCM_OK;
}

static GasPar gas_par(const gcm_gas_radiation_par &g) {
    GasPar p;
    p.k_h2o_lw = g.k_h2o_lw; p.k_co2_lw = g.k_co2_lw; p.k_h2o_sw = g.k_h2o_sw; p.k_co2_sw = g.k_co2_sw;
    p.co2 = g.co2_vmr * (kGasMco2 * 1e-3) / (kGasMd * 1e-3);  // mmr_from_vmr, grey_solar.py:21-29, molar masses in kg / mol
    p.a_g = g.ground_albedo;
    p.same = g.k_h2o_lw == g.k_h2o_sw && g.k_co2_lw == g.k_co2_sw;
    return p;
}

// the insolation of every row: "uniform" S0 0.5 0.5 (grey_solar.py:208-209), "daily" daily_average_irradiance
// (grey_solar.py:32-36) with the arccos argument kept inside [-1, 1]
int gas_insolation(int kind, int nlat, const double *lat, double declination, double solar_constant, double *out, std::string *err) {
    const char *fn = "gcm_gas_insolation";
    const auto bad = [&](const char *what) { *err = std::string(fn) + ": " + what; return GCM_ERR_ARG; };
    if (nlat < 0 || (nlat > 0 && (!lat || !out))) return bad("nlat must be >= 0, lat and out are required");
    if (!std::isfinite(solar_constant) || solar_constant < 0.0) return bad("solar_constant must be finite and >= 0");
    if (!(std::fabs(declination) <= M_PI / 2)) return bad("declination must lie in [-pi/2, pi/2]");
    if (kind == GCM_INSOLATION_ZENITH) return bad("\"zenith\" has no row table: it depends on the longitude and the clock");
    if (kind != GCM_INSOLATION_UNIFORM && kind != GCM_INSOLATION_DAILY) return bad("unknown insolation");
    for (int j = 0; j < nlat; ++j) {
        if (kind == GCM_INSOLATION_UNIFORM) {
            out[j] = solar_constant * (0.5 * 0.5);
            continue;
        }
        if (!std::isfinite(lat[j])) return bad("lat must be finite");
        const double x = fmin(fmax(-std::tan(lat[j]) * std::tan(declination), -1.0), 1.0);
        const double dH = std::acos(x);
        out[j] = solar_constant / (M_PI * 1.0) *
                 (dH * std::sin(lat[j]) * std::sin(declination) + std::cos(lat[j]) * std::cos(declination) * std::sin(dH));
    }
    return GCM_OK;
}

int gas_radiation_columns(int ncol, int L, const gcm_gas_radiation_par *g, const double *SC, const double *p, double ptop,
                          const double *sig, const double *dsig, const double *tt, const double *q, const double *gt,
                          double *dt_ground, double *dt_air, double *olr, double *words, std::string *err) {
    const char *fn = "gcm_gas_radiation_columns";
    if (int rc = gas_radiation_check(g, fn, err)) return rc;
    if (ncol < 0 || L < 1 || !sig || !dsig || (ncol > 0 && (!SC || !p || !tt || !q || !gt))) {
        *err = std::string(fn) + ": ncol must be >= 0, L >= 1, SC, p, sig, dsig, tt, q and gt are required";
        return GCM_ERR_ARG;
    }
    const GasPar par = gas_par(*g);
    std::vector<double> park((size_t)L);
    const size_t n = (size_t)ncol;
    for (size_t i = 0; i < n; ++i) {
        const GasColumn c = gas_column(
            L, par, SC[i], gt[i],
            [&](int k) {
                GasLevelIn in;
                in.tp = p[i] * sig[k] + ptop;
                in.dp = p[i] * dsig[k];
                in.ex = 1.0;
                in.tt = tt[(size_t)k * n + i];
                in.q = q[(size_t)k * n + i];
                return in;
            },
            [&](int k) -> double & { return park[(size_t)k]; },
            [&](int k, double d, const GasLevelIn &) { if (dt_air) dt_air[(size_t)k * n + i] = d; });
        if (dt_ground) dt_ground[i] = c.dt_ground;
        if (olr) olr[i] = c.olr;
        if (words) {
            words[i] = SC[i]; words[n + i] = c.sw_sfc; words[2 * n + i] = c.lw_down; words[3 * n + i] = c.lw_up; words[4 * n + i] = c.olr;
        }
    }
    return GCM_OK;
}

// ---------------------------------------------------------------- the handle's side
bool pe25d_gas_radiation_on(const Pe25d *m) { return m->gas.on; }

// every stream a launch that reads the tables may still run on
static int gas_quiet(Pe25d *m, const char *fn, hipStream_t s, std::string *err) {
    if (int rc = hip_rc(hipStreamSynchronize(s), fn, err)) return rc;
    if (m->aux) return hip_rc(hipStreamSynchronize(m->aux), fn, err);
    return GCM_OK;
}

int pe25d_set_gas_radiation(Pe25d *m, const gcm_gas_radiation_par *g, hipStream_t s, std::string *err) {
    const char *fn = "gcm_set_gas_radiation";
    PeGasRad &z = m->gas;
    if (!g) {
        if (!z.on) return GCM_OK;
        if (int rc = gas_quiet(m, fn, s, err)) return rc;
        z.on = false;
        return GCM_OK;
    }
    if (int rc = gas_radiation_check(g, fn, err)) return rc;
    if (m->L > kGasMaxL) { *err = std::string(fn) + ": more levels than the kernel's LDS column holds"; return GCM_ERR_UNSUPPORTED; }
    if (!m->gt_set) { *err = std::string(fn) + ": set the ground temperature first (gcm_set_ground)"; return GCM_ERR_STATE; }
    z.par = *g;
    z.on = true;
    return GCM_OK;
}

const gcm_gas_radiation_par *pe25d_gas_radiation_par(const Pe25d *m) { return m->gas.on ? &m->gas.par : nullptr; }

// the lat / lon tables the grey radiation's kernel reads too (pe25d_physics_tables): uploaded when their content changes
static int gas_geo_tables(Pe25d *m, const double *lat, const double *lon, hipStream_t s, bool *changed, std::string *err) {
    const char *fn = "gas radiation";
    const int W = m->W, Hg = m->Hg;
    *changed = false;
    if (m->rad_geo && m->rad_latlon.size() == (size_t)Hg + W && !memcmp(m->rad_latlon.data(), lat, sizeof(double) * Hg) &&
        !memcmp(m->rad_latlon.data() + Hg, lon, sizeof(double) * W))
        return GCM_OK;
    if (int rc = gas_quiet(m, fn, s, err)) return rc;
    m->rad_latlon.assign(lat, lat + Hg);
    m->rad_latlon.insert(m->rad_latlon.end(), lon, lon + W);
    std::vector<double> &Gt = m->rad_geo_host;
    Gt.assign((size_t)2 * Hg + W, 0.0);
    for (int j = 0; j < Hg; ++j) { Gt[j] = std::cos(lat[j]); Gt[Hg + j] = std::sin(lat[j]); }
    for (int i = 0; i < W; ++i) Gt[2 * Hg + i] = lon[i];
    if (!m->rad_geo && !dev_upload<double>(m, &m->rad_geo, nullptr, Gt.size())) {
        *err = "hip: gas radiation geometry allocation failed"; return GCM_ERR_HIP;
    }
    *changed = true;
    return hip_rc(hipMemcpy(m->rad_geo, Gt.data(), sizeof(double) * Gt.size(), hipMemcpyHostToDevice), fn, err);
}

// what a launch with the parameters g reads, in place when the call returns: the level table, the lat / lon tables and,
// for "uniform" and "daily", the insolation of every global row
int pe25d_gas_radiation_tables(Pe25d *m, const gcm_gas_radiation_par *g, const double *lat, const double *lon, hipStream_t s,
                               std::string *err) {
    const char *fn = "gas radiation";
    PeGasRad &z = m->gas;
    if (!m->gt_set) { *err = "gas radiation: set the ground temperature first (gcm_set_ground)"; return GCM_ERR_STATE; }
    if (!lat || !lon) { *err = "gas radiation: lat and lon tables are required"; return GCM_ERR_ARG; }
    if (m->L > kGasMaxL) { *err = "gas radiation: more levels than the kernel's LDS column holds"; return GCM_ERR_UNSUPPORTED; }
    if (!pe25d_level_table(m, fn, err)) return GCM_ERR_HIP;
    bool geo = false;
    if (int rc = gas_geo_tables(m, lat, lon, s, &geo, err)) return rc;
    if (g->insolation == GCM_INSOLATION_ZENITH) return GCM_OK;
    if (z.sc_row && !geo && z.key_kind == g->insolation && z.key[0] == g->declination && z.key[1] == g->solar_constant) return GCM_OK;
    std::vector<double> fresh((size_t)m->Hg);
    if (int rc = gas_insolation(g->insolation, m->Hg, lat, g->declination, g->solar_constant, fresh.data(), err)) return rc;
    if (int rc = gas_quiet(m, fn, s, err)) return rc;
    if (!z.sc_row && !dev_upload<double>(m, &z.sc_row, nullptr, fresh.size())) {
        *err = "hip: gas radiation insolation table allocation failed"; return GCM_ERR_HIP;
    }
    if (int rc = hip_rc(hipMemcpy(z.sc_row, fresh.data(), sizeof(double) * fresh.size(), hipMemcpyHostToDevice), fn, err)) {
        z.key_kind = -1;
        return rc;
    }
    z.key_kind = g->insolation; z.key[0] = g->declination; z.key[1] = g->solar_constant;
    return GCM_OK;
}

// rows [j0, j1) and [jb0, jb1) of state set `set` (a band's ghost rows: negative, or >= H); keep_ghosts and the
// bookkeeping behind a theta written in place: as radiation_launch (pe25d_physics.hip)
template <typename T>
static int gas_launch(Pe25d *m, const gcm_gas_radiation_par &g, int set, int j0, int j1, int jb0, int jb1, bool keep_ghosts, bool apply,
                      bool budget, double dt, double utc, double *dt_air_host, double *dtg_host, double *olr_host, hipStream_t s,
                      std::string *err) {
    const char *fn = "gas radiation";
    PeBufs<T> &B = bufs<T>(m);
    PeGasRad &z = m->gas;
    const int W = m->W, L = m->L, Hg = m->Hg;
    const int n0 = std::max(0, j1 - j0), nrows = n0 + std::max(0, jb1 - jb0);
    if (nrows <= 0) return GCM_OK;
    if (j0 < -kGhost || j1 > m->H + kGhost || (jb1 > jb0 && (jb0 < -kGhost || jb1 > m->H + kGhost))) {
        *err = "gas radiation: rows outside the handle's allocation"; return GCM_ERR_ARG;
    }
    const bool zenith = g.insolation == GCM_INSOLATION_ZENITH;
    if (!m->lev_tab || !m->rad_geo || (!zenith && !z.sc_row)) { *err = "gas radiation: no tables in place"; return GCM_ERR_STATE; }
    GasArgsT<T> a{};
    a.p = B.st[set][GCM_P]; a.q = B.st[set][GCM_Q]; a.t = B.st[set][GCM_T];
    a.exner_tab = m->exner_tab;
    a.sig = m->lev_tab; a.dsig = m->lev_tab + L;
    a.coslat = m->rad_geo; a.sinlat = m->rad_geo + Hg; a.lon = m->rad_geo + 2 * Hg;
    a.sc_row = z.sc_row;
    a.gt = m->gt;
    a.par = gas_par(g);
    a.S0 = g.solar_constant; a.sin_d = std::sin(g.declination); a.cos_d = std::cos(g.declination);
    a.hour_angle = utc / (-24 * 3600.0) * 360 * (M_PI / 180);      // grey_solar.py:51
    a.dt = dt; a.ptop = m->cfg.ptop;
    a.zenith = zenith ? 1 : 0; a.apply = apply ? 1 : 0;
    a.W = W; a.L = L; a.Hg = Hg; a.row0 = m->cfg.row0;
    a.j0 = j0; a.n0 = n0; a.jb0 = jb0;
    if (!apply) {
        if (!z.diag && !dev_upload<double>(m, &z.diag, nullptr, (size_t)2 * m->H * W)) {
            *err = "hip: gas radiation diagnostic allocation failed"; return GCM_ERR_HIP;
        }
        a.dt_air = B.pgfu; a.dtg = z.diag; a.olr = z.diag + (size_t)m->H * W;
    }
    if (budget) {
        a.bud = pe25d_slab_ocean_word(m, GCM_SLAB_SC);
        a.bud_stride = (long)rows_alloc(m) * W;
        if (!a.bud) { *err = "gas radiation: no slab ocean registered for the budget launch"; return GCM_ERR_STATE; }
    }
    const size_t lds = sizeof(double) * (size_t)L * kGasLanes;
    const void *fnp = budget ? (const void *)pe_gas_radiation_kernel<T, true> : (const void *)pe_gas_radiation_kernel<T, false>;
    if (z.lds_set[budget ? 1 : 0] != (int)lds) {
        if (int rc = hip_rc(hipFuncSetAttribute(fnp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), fn, err)) return rc;
        z.lds_set[budget ? 1 : 0] = (int)lds;
    }
    if (apply && !keep_ghosts) m->ghost_ready = -1;        // theta changes in place
    m->last_stage_set = -1;                                // gcm_get_intermediate: theta changed, or pgfu holds the tendencies
    if (!(apply && (keep_ghosts || m->wrap))) m->k4_fork_valid = false;
    const dim3 gg((unsigned)((W + kGasLanes - 1) / kGasLanes), (unsigned)nrows);
    if (budget) hipLaunchKernelGGL((pe_gas_radiation_kernel<T, true>), gg, dim3(kGasLanes), lds, s, a);
    else hipLaunchKernelGGL((pe_gas_radiation_kernel<T, false>), gg, dim3(kGasLanes), lds, s, a);
    if (hipGetLastError() != hipSuccess) { *err = "hip: gas radiation kernel launch failed"; return GCM_ERR_HIP; }
    if (apply) return GCM_OK;                              // stays asynchronous on `s`
    const size_t cells = sizeof(double) * (size_t)m->H * W;
    if (dt_air_host && field_to_host(m, dt_air_host, B.pgfu, L, s) != hipSuccess) { *err = "hip: dt_air copy-back failed"; return GCM_ERR_HIP; }
    if (dtg_host && hipMemcpyAsync(dtg_host, a.dtg, cells, hipMemcpyDeviceToHost, s) != hipSuccess) { *err = "hip: dt_ground copy-back failed"; return GCM_ERR_HIP; }
    if (olr_host && hipMemcpyAsync(olr_host, a.olr, cells, hipMemcpyDeviceToHost, s) != hipSuccess) { *err = "hip: olr copy-back failed"; return GCM_ERR_HIP; }
    return hip_rc(hipStreamSynchronize(s), fn, err);
}

// the registered phase in the solar slot of a step (pe25d_solar_rows): in place, BUDGET while the slab ocean is registered
int pe25d_gas_radiation_rows(Pe25d *m, int set, int j0, int j1, int jb0, int jb1, bool keep_ghosts, double dt, double utc, hipStream_t s,
                             std::string *err) {
    if (!m->gas.on) { *err = "gas radiation: not registered (gcm_set_gas_radiation)"; return GCM_ERR_STATE; }
    if (set < 0) set = m->cur_i;
    const bool budget = m->slab.on;
    return m->f32 ? gas_launch<float>(m, m->gas.par, set, j0, j1, jb0, jb1, keep_ghosts, true, budget, dt, utc, nullptr, nullptr, nullptr, s, err)
                  : gas_launch<double>(m, m->gas.par, set, j0, j1, jb0, jb1, keep_ghosts, true, budget, dt, utc, nullptr, nullptr, nullptr, s, err);
}

// gcm_gas_radiation (diagnostic) and gcm_gas_radiation_step (in place; on a band the ghost rows too, as pe25d_radiation)
int pe25d_gas_radiation(Pe25d *m, bool apply, double dt, double utc, const gcm_gas_radiation_par *g, const double *lat, const double *lon,
                        double *dtg_host, double *dt_air_host, double *olr_host, hipStream_t s, std::string *err) {
    if (int rc = pe25d_gas_radiation_tables(m, g, lat, lon, s, err)) return rc;
    const int gh = (apply && !m->wrap) ? kGhost : 0;
    return m->f32 ? gas_launch<float>(m, *g, m->cur_i, -gh, m->H + gh, 0, 0, false, apply, false, dt, utc, dt_air_host, dtg_host, olr_host, s, err)
                  : gas_launch<double>(m, *g, m->cur_i, -gh, m->H + gh, 0, 0, false, apply, false, dt, utc, dt_air_host, dtg_host, olr_host, s, err);
}

}  // namespace gcm

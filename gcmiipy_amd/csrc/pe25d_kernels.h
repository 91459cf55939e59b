// 2.5-D sigma-level primitive equations (GCM_PE25D): host-visible interface of
// pe25d_kernels.hip (the stage), pe25d_state.hip, pe25d_physics.hip, pe25d_diag.hip, pe25d_held_suarez.hip,
// pe25d_climate.hip, pe25d_plev.hip, pe25d_plev_height.hip, pe25d_spectra.hip, pe25d_moist.hip, pe25d_convect.hip, pe25d_betts_miller.hip, pe25d_convect_tracers.hip, pe25d_boundary_layer.hip, pe25d_slab_ocean.hip, pe25d_gas_radiation.hip and pe25d_tracers.hip (the passive tracers), used by gcmcore.hip, gcm_band.hip, gcm_diag.hip and gcm_pe.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/gcmcore.h"

namespace gcm {

struct Pe25d;
struct SegCopy;   // sw2d_kernels.h

Pe25d *pe25d_create(const gcm_config &cfg, hipStream_t s, std::string *err);
void pe25d_destroy(Pe25d *m);
int pe25d_set(Pe25d *m, bool star, const double *p, const double *u, const double *v,
              const double *t, const double *q, hipStream_t s, std::string *err);
int pe25d_get(Pe25d *m, bool star, double *p, double *u, double *v, double *t, double *q,
              hipStream_t s, std::string *err);
int pe25d_step(Pe25d *m, double dt, hipStream_t s, std::string *err);
int pe25d_step_part(Pe25d *m, int part, double dt, hipStream_t s, std::string *err);
// chained: the call belongs to gcm_band_run's own sequence (the library knows everything queued between two stages)
int pe25d_step_phase(Pe25d *m, int phase, double dt, hipStream_t s, std::string *err, bool chained = false);
int pe25d_set_halo_buffers(Pe25d *m, void *north, void *south, hipStream_t s, std::string *err);
int pe25d_wait_edges(Pe25d *m, hipStream_t s, std::string *err);
int pe25d_prep_ghost_rows(Pe25d *m, std::string *err);   // gcm_band_run: behind the unpack on the second stream
hipStream_t pe25d_aux_stream(const Pe25d *m);
void pe25d_join_third_stream(Pe25d *m, hipStream_t s);
void pe25d_fork_invalidate(Pe25d *m);
void pe25d_set_edges_first(Pe25d *m, bool on);   // gcm_set_band_overlap on a GCM_PE25D band
// a new non-blocking stream that demonstrably runs beside `main` (and `other`, may be null)
hipStream_t concurrent_stream(hipStream_t main, hipStream_t other);
void launch_spin(hipStream_t s, double us);   // GCM_BAND_EXCHANGE_DELAY_US: the loopback exchange takes that long
int pe25d_half(Pe25d *m, int stage, double dt, hipStream_t s, std::string *err);
size_t pe25d_halo_bytes(const Pe25d *m);
int pe25d_halo_segments(Pe25d *m, bool pack, int side, void *dev_buf, SegCopy *c, std::string *err);
int pe25d_ground(Pe25d *m, bool set, const double *in, double *out, hipStream_t s, std::string *err);
int pe25d_intermediate(Pe25d *m, int kind, double *out, hipStream_t s, std::string *err);
int pe25d_filter_field(Pe25d *m, int nlev, const double *in, double *out, hipStream_t s, std::string *err);
int pe25d_radiation(Pe25d *m, bool apply, double dt, double utc, double t_lw, double t_sw, double albedo,
                    const double *lat, const double *lon, double *dTdt_host, double *dtg_host,
                    hipStream_t s, std::string *err);
// grey_check: the accepted parameters (GCM_ERR_ARG and "<fn>: <what>" otherwise; dsig may be null: the levels'
// transmissivities are then not checked); grey_radiation_tables: gcm_grey_radiation_tables (no handle, no device), the
// builder pe25d_physics_tables uploads from
int grey_check(int L, const double *dsig, double t_lw, double t_sw, double albedo, const char *fn, std::string *err);
int grey_radiation_tables(int L, const double *dsig, const double *sig, double t_lw, double t_sw, double *out, std::string *err);
int pe25d_grey_check(const Pe25d *m, double t_lw, double t_sw, double albedo, const char *fn, std::string *err);
int pe25d_physics_tables(Pe25d *m, double t_lw, double t_sw, const double *lat, const double *lon, hipStream_t s,
                         std::string *err);
int pe25d_solar_rows(Pe25d *m, int set, int j0, int j1, int jb0, int jb1, bool keep_ghosts, double dt, double utc, double albedo,
                     hipStream_t s, std::string *err);
// Held-Suarez forcing (pe25d_held_suarez.hip).  held_suarez_tables: gcm_held_suarez_tables (no handle, no device);
// pe25d_hs_tables: the device tables for (hs, dt), built and uploaded when either changed (hs->lat: [global_height]);
// pe25d_hs_rows: the kernel over rows [j0, j1) and [jb0, jb1) of state set `set` (-1: the current one) on `s`, tables in
// place; keep_ghosts as for pe25d_solar_rows
int held_suarez_tables(int L, const double *sig, int nlat, const double *lat, const gcm_held_suarez *hs, double dt,
                       double *fu, double *kt, double *s2, double *c2, std::string *err);
int held_suarez_check(const gcm_held_suarez *hs, const char *fn, std::string *err);
int pe25d_hs_tables(Pe25d *m, const gcm_held_suarez *hs, double dt, hipStream_t s, std::string *err);
int pe25d_hs_rows(Pe25d *m, int set, int j0, int j1, int jb0, int jb1, bool keep_ghosts, hipStream_t s, std::string *err);
// The four sampled diagnostics, in the order a step samples.  What they share is one set of routines over a PeSampler
// (pe25d_state.hip), on `s`, the caller's stream.  pe25d_sampler_registered: GCM_ERR_STATE and "<fn>: no <what> registered
// (gcm_set_<name>)" without a registration, the one place that forms that message; every: the interval, 0 without one;
// due: counts one step of gcm_step / gcm_band_run, true where that step ends with a sample; reset, get and put are
// gcm_<name>_reset, gcm_get_<name> and gcm_put_<name> -- get takes null pointers, put needs every array the diagnostic
// has (b: the second block of the climatology and the maps, else null) and nsamples >= 0, and synchronises `s` behind its
// copies whether or not one failed: the caller's arrays are free when it returns; free: the buffer off the handle's list
// and freed, the sampler cleared (a unit's pe25d_set_* calls it).  What stays with each unit: pe25d_set_* (the rules of
// a second registration differ), *_sample (arguments and launch) and *_plan.
//
// A sample and the stages that follow it.  Every sample is a pure reader of the current state set on `s` and writes its
// own sums only: it leaves the column sums, the fork at the last K4 and the ghost-row bookkeeping as they are (unlike
// pe25d_hs_rows, which writes u and v).  What must still hold is that whatever overwrites this state set later is
// ordered behind the launch.  The set is written again by the corrector's K4 two steps on, by the physics phases behind
// it, and -- a band -- by the unpack of the exchange that follows that K4 (its ghost rows, of which a sample reads v's
// row -1, the first north ghost row).  K4 of the rows the caller's stream keeps (all rows; a band: the interior rows)
// follows the launch in stream order on `s`.  A band's edge rows' K4 runs on the second stream, which every stage makes
// wait for its fork: the completion of the previous stage's K4 on `s` (ev_k4) or a record on `s` at the head of the
// stage (ev_fork) -- an event behind the launch on `s` in either case, from the very next stage on; the pack, the
// exchange and the unpack follow that K4 in stream order (or on streams that wait for the pack).  The third stream
// writes no state set.  The launches of the next stage that may run beside a sample (chain B forked at ev_k4: K1, pit,
// column sums, anchors, the tracers) write intermediates and tracers only, none of which a sample reads; q is a state
// field, not a tracer.  The samples of one step follow each other on `s` and write their own sums only.
enum PeSample { kSampleClimate, kSamplePlevClimate, kSampleSpectra, kSamplePlevMaps };
int pe25d_sampler_registered(const Pe25d *m, PeSample of, const char *fn, std::string *err);
int pe25d_sampler_every(const Pe25d *m, PeSample of);
bool pe25d_sampler_due(Pe25d *m, PeSample of);
int pe25d_sampler_reset(Pe25d *m, PeSample of, hipStream_t s, std::string *err);
int pe25d_sampler_get(Pe25d *m, PeSample of, double *a, double *b, int64_t *nsamples, hipStream_t s, std::string *err);
int pe25d_sampler_put(Pe25d *m, PeSample of, const double *a, const double *b, int64_t nsamples, hipStream_t s, std::string *err);
void pe25d_sampler_free(Pe25d *m, PeSample of);
// Zonal-mean climatology (pe25d_climate.hip): gcm_set_climate and gcm_climate_sample
int pe25d_set_climate(Pe25d *m, int every, hipStream_t s, std::string *err);
int pe25d_climate_sample(Pe25d *m, hipStream_t s, std::string *err);
// Pressure levels (pe25d_plev.hip).  plev_columns: no handle, no device (gcm_plev_columns).  pe25d_plev_fields:
// gcm_plev_fields on `s`, synchronised before it returns.  gcm_set_plev_climate, gcm_plev_climate_sample and
// gcm_plev_climate_plan.  pe25d_plev_levels: the registered targets of the climatology or of the maps
// (gcm_plev_climate_levels, gcm_plev_maps_levels), at most cap of them into P (may be null) -> their number
int plev_columns(int ncol, int L, int N, const double *pl, const double *x, const double *P, double *out, int *valid, std::string *err);
int pe25d_plev_fields(Pe25d *m, int N, const double *P, double fill, double *out, int32_t *valid, hipStream_t s, std::string *err);
int pe25d_set_plev_climate(Pe25d *m, int every, int N, const double *P, hipStream_t s, std::string *err);
int pe25d_plev_levels(const Pe25d *m, PeSample of, double *P, int cap);
int pe25d_plev_climate_plan(const Pe25d *m, int *out, int nout);
int pe25d_plev_climate_sample(Pe25d *m, hipStream_t s, std::string *err);
// Geopotential height on pressure levels and time-mean maps (pe25d_plev_height.hip).  plev_height_columns: no handle, no
// device (gcm_plev_height_columns).  pe25d_plev_height: gcm_plev_height on `s`, synchronised before it returns.
// gcm_set_plev_maps, gcm_plev_maps_sample and gcm_plev_maps_plan
int plev_height_columns(int ncol, int L, int N, const double *p, const double *theta, const double *hmG, const double *sig,
                        const double *dsig, const double *sigt, double ptop, const double *P, double *out, int *valid, std::string *err);
int pe25d_plev_height(Pe25d *m, int N, const double *P, double fill, double *out, int32_t *valid, hipStream_t s, std::string *err);
int pe25d_set_plev_maps(Pe25d *m, int every, int N, const double *P, hipStream_t s, std::string *err);
int pe25d_plev_maps_plan(const Pe25d *m, int *out, int nout);
int pe25d_plev_maps_sample(Pe25d *m, hipStream_t s, std::string *err);
// Zonal wavenumber spectra (pe25d_spectra.hip): gcm_set_spectra, gcm_spectra_sample and gcm_spectra_plan;
// pe25d_spectra_mmax: the registered mmax (gcm_spectra_mmax)
int pe25d_set_spectra(Pe25d *m, int every, int mmax, hipStream_t s, std::string *err);
int pe25d_spectra_mmax(const Pe25d *m);
int pe25d_spectra_plan(const Pe25d *m, int *out, int nout);
int pe25d_spectra_sample(Pe25d *m, hipStream_t s, std::string *err);
// The column sums of the convective adjustment (count, levels), of the moist physics (precip, evap), of the boundary
// layer (shf, evap) and of the Betts-Miller convection (precip, count), one set of routines for all (pe25d_state.hip), on `s`, the caller's stream.  pe25d_sums_set: allocated and zeroed (on) or freed;
// a phase is registered where its sums are in place, and pe25d_sums_on is the one place that says so.  reset, get and
// put are gcm_<phase>_reset, gcm_get_<phase> and gcm_put_<phase>: GCM_ERR_STATE where the phase is not registered
enum PeSums { kSumsConvect, kSumsMoist, kSumsBoundary, kSumsBettsMiller };
int pe25d_sums_set(Pe25d *m, PeSums of, bool on, hipStream_t s, std::string *err);
bool pe25d_sums_on(const Pe25d *m, PeSums of);
int pe25d_sums_reset(Pe25d *m, PeSums of, hipStream_t s, std::string *err);
int pe25d_sums_get(Pe25d *m, PeSums of, double *a, double *b, double *seconds, int64_t *nsteps, hipStream_t s, std::string *err);
int pe25d_sums_put(Pe25d *m, PeSums of, const double *a, const double *b, double seconds, int64_t nsteps, hipStream_t s, std::string *err);
// Moist physics (pe25d_moist.hip).  moist_check / moist_saturation_table: no handle, no device (gcm_moist_saturation).
// pe25d_moist_tables: the level tables in place and (mo, dt) as the parameters of the launches that follow;
// pe25d_moist_rows: the kernel over rows [j0, j1) and [jb0, jb1) of state set `set` (-1: the current one) on `s`;
// keep_ghosts as for pe25d_solar_rows; accumulate: the own rows' precipitation and evaporation go to the registered sums
// and the call counts as one application of dt
int moist_check(const gcm_moist *mo, const char *fn, std::string *err);
int moist_saturation_table(int n, const double *T, const double *p_lev, double *q_s, double *dq_s, int *can, std::string *err);
int pe25d_moist_tables(Pe25d *m, const gcm_moist *mo, double dt, std::string *err);
int pe25d_moist_rows(Pe25d *m, int set, int j0, int j1, int jb0, int jb1, bool keep_ghosts, bool accumulate, hipStream_t s,
                     std::string *err);
// Convective adjustment (pe25d_convect.hip).  convect_check / convect_columns: no handle, no device (gcm_convect_columns).
// pe25d_convect_fits: ahead of pe25d_sums_set(kSumsConvect, on); GCM_ERR_UNSUPPORTED where the block stack of the handle's
// L does not fit a workgroup's LDS; pe25d_convect_tables: the level tables in place and cv as the parameters of the
// launches that follow, dt what an accumulating launch adds to the seconds; pe25d_convect_rows: the kernel over rows
// [j0, j1) and [jb0, jb1) of state set `set` (-1: the current one) on `s`; keep_ghosts as for pe25d_solar_rows;
// accumulate: the own rows' counts go to the registered sums and the call counts as one application
int convect_check(const gcm_convect *cv, const char *fn, std::string *err);
int convect_columns(int ncol, int L, const double *y, const double *w, const double *q, const double *dsig, int mix_q,
                    double *y_out, double *q_out, int32_t *nblock, std::string *err);
int pe25d_convect_fits(Pe25d *m, const char *fn, std::string *err);
int pe25d_convect_tables(Pe25d *m, const gcm_convect *cv, double dt, std::string *err);
int pe25d_convect_rows(Pe25d *m, int set, int j0, int j1, int jb0, int jb1, bool keep_ghosts, bool accumulate, hipStream_t s,
                       std::string *err);
// Betts-Miller convection (pe25d_betts_miller.hip).  betts_miller_check / betts_miller_columns: no handle, no device
// (gcm_betts_miller_columns).  pe25d_betts_miller_fits: ahead of pe25d_sums_set(kSumsBettsMiller, on); GCM_ERR_UNSUPPORTED
// for L < 2, a sig table that does not strictly decrease and an L whose parked changes do not fit a workgroup's LDS;
// pe25d_betts_miller_tables: the level tables in place and (bm, dt) as the parameters of the launches that follow;
// pe25d_betts_miller_rows: the kernel over rows [j0, j1) and [jb0, jb1) of state set `set` (-1: the current one) on `s`;
// keep_ghosts as for pe25d_solar_rows; accumulate: the own rows' precipitation and counts go to the registered sums and
// the call counts as one application of dt
int betts_miller_check(const gcm_betts_miller *bm, const char *fn, std::string *err);
int betts_miller_columns(int ncol, int L, const double *p, const double *theta, const double *q, const double *sig,
                         const double *dsig, double ptop, double dt, const gcm_betts_miller *bm, double *theta_out,
                         double *q_out, double *precip, int32_t *kt, int32_t *k_lcl, double *margin, std::string *err);
int pe25d_betts_miller_fits(Pe25d *m, const char *fn, std::string *err);
int pe25d_betts_miller_tables(Pe25d *m, const gcm_betts_miller *bm, double dt, std::string *err);
int pe25d_betts_miller_rows(Pe25d *m, int set, int j0, int j1, int jb0, int jb1, bool keep_ghosts, bool accumulate,
                            hipStream_t s, std::string *err);
// Surface fluxes and boundary-layer mixing (pe25d_boundary_layer.hip).  boundary_layer_check / _surface / _column: no
// handle, no device (gcm_boundary_layer_surface, gcm_boundary_layer_column).  pe25d_boundary_layer_fits: what a
// registration or a step needs of the handle -- a single domain or a band that has opted in
// (pe25d_set_band_boundary_layer: gcm_set_band_boundary_layer; GCM_ERR_STATE for on = false while the phase is
// registered), L >= 2, sig decreasing in k (GCM_ERR_UNSUPPORTED), a ground temperature (GCM_ERR_STATE);
// pe25d_boundary_layer_scratch: the float64 scratch fields in place or freed;
// pe25d_boundary_layer_tables: the checks above, the level tables and the scratch in place and (bl, dt) as the
// parameters of the launches that follow; pe25d_boundary_layer_rows: the two launches over every row of state set `set`
// (-1: the current one) of a single domain, over the own rows of a band (ghost rows -1 and H current), on `s`;
// accumulate: the surface's heat and water go to the registered sums and the call counts
// as one application of dt
int boundary_layer_check(const gcm_boundary_layer *bl, const char *fn, std::string *err);
int boundary_layer_surface(int n, const gcm_boundary_layer *bl, double ptop, double sig0, const double *uc, const double *vc,
                           const double *theta0, const double *q0, const double *p, double *S, double *z_a, double *cd,
                           std::string *err);
int boundary_layer_column(int ncol, int L, const double *dsig, const double *a, const double *x, const double *target,
                          const double *X, double *X_out, double *X0_surface, std::string *err);
int pe25d_set_band_boundary_layer(Pe25d *m, bool on, std::string *err);
bool pe25d_band_boundary_layer(const Pe25d *m);
int pe25d_boundary_layer_fits(Pe25d *m, const char *fn, std::string *err);
int pe25d_boundary_layer_scratch(Pe25d *m, bool on, hipStream_t s, std::string *err);
int pe25d_boundary_layer_tables(Pe25d *m, const gcm_boundary_layer *bl, double dt, hipStream_t s, std::string *err);
int pe25d_boundary_layer_rows(Pe25d *m, int set, bool keep_ghosts, bool accumulate, hipStream_t s, std::string *err);
// Slab mixed-layer ocean (pe25d_slab_ocean.hip).  slab_ocean_check / slab_ocean_cells: no handle, no device
// (gcm_slab_ocean_cells).  pe25d_set_slab_ocean: gcm_set_slab_ocean (so == nullptr: off, words, sums and fields freed;
// GCM_ERR_STATE without a ground temperature); pe25d_slab_ocean_on: the registration, the one place that says so;
// pe25d_slab_ocean_word: flux word n (GCM_SLAB_*) at interior row 0, null without a registration -- what the radiation's
// launch and the boundary layer's store into; pe25d_slab_ocean_rows: the registered slab over rows [j0, j1) and
// [jb0, jb1) on `s` with the step dt, `radiation` / `boundary`: whether that phase stored its words in this step (else
// they count, and are stored, as zero), accumulate: the own rows' terms go to the sums and the call counts as one
// application of dt; apply, fluxes, get, put and reset are gcm_slab_ocean_apply, gcm_get_slab_ocean_fluxes,
// gcm_get_slab_ocean, gcm_put_slab_ocean and gcm_slab_ocean_reset
int slab_ocean_check(const gcm_slab_ocean *so, const char *fn, std::string *err);
int slab_ocean_cells(int n, const gcm_slab_ocean *so, double dt, const double *gt, const double *C, const double *words,
                     const double *Q, double *gt_out, double *E4_out, std::string *err);
int pe25d_set_slab_ocean(Pe25d *m, const gcm_slab_ocean *so, const double *cap, const double *qflux, hipStream_t s, std::string *err);
bool pe25d_slab_ocean_on(const Pe25d *m);
double *pe25d_slab_ocean_word(const Pe25d *m, int n);
int pe25d_slab_ocean_rows(Pe25d *m, int j0, int j1, int jb0, int jb1, double dt, bool radiation, bool boundary, bool accumulate,
                          hipStream_t s, std::string *err);
int pe25d_slab_ocean_apply(Pe25d *m, double dt, const gcm_slab_ocean *so, const double *words, hipStream_t s, std::string *err);
int pe25d_slab_ocean_fluxes(Pe25d *m, double *words, hipStream_t s, std::string *err);
int pe25d_slab_ocean_get(Pe25d *m, double *sums, double *seconds, int64_t *nsteps, hipStream_t s, std::string *err);
int pe25d_slab_ocean_put(Pe25d *m, const double *sums, double seconds, int64_t nsteps, hipStream_t s, std::string *err);
int pe25d_slab_ocean_reset(Pe25d *m, hipStream_t s, std::string *err);
// Grey radiation by water vapour and CO2 (pe25d_gas_radiation.hip).  gas_radiation_check / gas_insolation /
// gas_radiation_columns: no handle, no device (gcm_gas_insolation, gcm_gas_radiation_columns).  pe25d_set_gas_radiation:
// gcm_set_gas_radiation (g == nullptr: off; GCM_ERR_STATE without a ground temperature); pe25d_gas_radiation_on /
// pe25d_gas_radiation_par: the registration (null: none); pe25d_gas_radiation_tables: what a launch with g reads, in place;
// pe25d_gas_radiation_rows: the registered phase in place over rows [j0, j1) and [jb0, jb1) of state set `set` (-1: the
// current one) on `s` at the clock utc, keep_ghosts as for pe25d_solar_rows, which forwards to it while a registration
// stands; pe25d_gas_radiation: gcm_gas_radiation (apply false; any output may be null) and gcm_gas_radiation_step
int gas_radiation_check(const gcm_gas_radiation_par *g, const char *fn, std::string *err);
int gas_insolation(int kind, int nlat, const double *lat, double declination, double solar_constant, double *out, std::string *err);
int gas_radiation_columns(int ncol, int L, const gcm_gas_radiation_par *g, const double *SC, const double *p, double ptop,
                          const double *sig, const double *dsig, const double *tt, const double *q, const double *gt,
                          double *dt_ground, double *dt_air, double *olr, double *words, std::string *err);
int pe25d_set_gas_radiation(Pe25d *m, const gcm_gas_radiation_par *g, hipStream_t s, std::string *err);
bool pe25d_gas_radiation_on(const Pe25d *m);
const gcm_gas_radiation_par *pe25d_gas_radiation_par(const Pe25d *m);
int pe25d_gas_radiation_tables(Pe25d *m, const gcm_gas_radiation_par *g, const double *lat, const double *lon, hipStream_t s,
                               std::string *err);
int pe25d_gas_radiation_rows(Pe25d *m, int set, int j0, int j1, int jb0, int jb1, bool keep_ghosts, double dt, double utc, hipStream_t s,
                             std::string *err);
int pe25d_gas_radiation(Pe25d *m, bool apply, double dt, double utc, const gcm_gas_radiation_par *g, const double *lat, const double *lon,
                        double *dtg_host, double *dt_air_host, double *olr_host, hipStream_t s, std::string *err);
// Horizontal diffusion (pe25d_hdiff.hip).  hdiff_check / hdiff_tables / hdiff_apply: no handle, no device
// (gcm_hdiff_tables, gcm_hdiff_apply).  pe25d_hdiff_fits: what a registration or a step needs of the handle -- a single
// domain, W >= 4 and H >= 4, or a band that has opted in (GCM_ERR_UNSUPPORTED); pe25d_set_hdiff: gcm_set_hdiff (d == nullptr: off, the landing fields
// and tables freed); pe25d_hdiff_on / pe25d_hdiff_par: the registration; pe25d_hdiff_tables: the device tables for (d, dt),
// built and uploaded when either changed, and the landing fields of d's fields in place; pe25d_hdiff_rows: the launch
// over every row of state set `set` (-1: the current one) into the landing fields and their way back into the state,
// on `s`, tables in place; pe25d_hdiff_plan: gcm_hdiff_plan
int hdiff_check(const gcm_hdiff *d, const char *fn, std::string *err);
int hdiff_tables(int H, const double *dx_j, const double *dx_h, double dy, const gcm_hdiff *d, double dt, double *out, std::string *err);
int hdiff_apply(int H, int W, int nlev, const double *tab4, int order, const double *X, double *out, std::string *err);
int pe25d_hdiff_fits(const Pe25d *m, const char *fn, std::string *err);
int pe25d_set_hdiff(Pe25d *m, const gcm_hdiff *d, hipStream_t s, std::string *err);
bool pe25d_hdiff_on(const Pe25d *m);
const gcm_hdiff *pe25d_hdiff_par(const Pe25d *m);
int pe25d_hdiff_tables(Pe25d *m, const gcm_hdiff *d, double dt, hipStream_t s, std::string *err);
int pe25d_hdiff_rows(Pe25d *m, int set, bool keep_ghosts, hipStream_t s, std::string *err);
int pe25d_hdiff_plan(const Pe25d *m, int *out, int nout);
// A latitude band (pe25d_set_band_hdiff: gcm_set_band_hdiff; GCM_ERR_STATE for on = false while the phase is registered,
// GCM_ERR_UNSUPPORTED for on = true on a single domain) takes the band form of the kernel over its own rows, from the
// ghost rows as they are; the ghost rows of the selected fields are stale behind it.  hdiff_apply_band: the host build
// of that walk (gcm_hdiff_apply_band); hdiff_band_tables: a band's [8][Hb + 4] tables gathered from the global ones;
// pe25d_band_hdiff_done: gcm_end_step_diffuse was called for the step gcm_end_step_begin is about to end
int hdiff_apply_band(int Hb, int W, int nlev, const double *tab4, int order, const double *X, double *out, std::string *err);
void hdiff_band_tables(int Hg, int row0, int Hb, const double *glob, double *out);
int pe25d_set_band_hdiff(Pe25d *m, bool on, std::string *err);
bool pe25d_band_hdiff(const Pe25d *m);
bool pe25d_band_hdiff_done(const Pe25d *m);
void pe25d_set_band_hdiff_done(Pe25d *m, bool done);
int pe25d_new_state_set(const Pe25d *m);    // the set a corrector stage in flight writes (before the swap), else the current one
int pe25d_stats(Pe25d *m, const double *area_host, int area_len, double out[9], hipStream_t s, std::string *err);
int pe25d_filter_plan(int n, unsigned *out, int cap);   // gcm_filter_plan
// gcm_pe25d_phase_plan: pe25d_phase_geometry.h's query at the handle's own W, L, element size and compute units
int pe25d_phase_plan(const Pe25d *m, int phase, int rows, bool accumulate, int *out, int nout);
// gcm_pe25d_stage_plan: what a stage of the handle launches (pe25d_stage_geometry.h at the handle's own sizes and switches)
int pe25d_stage_plan(const Pe25d *m, int *out, int nout);
void pe25d_tv_shape(const Pe25d *m, int field, long *n_outer, long *n_axis, long *n_inner, int *wrap);
const void *pe25d_field(Pe25d *m, int field, long *n, int *f32);
// passive tracers: c / the result [n][L][H][W] float64 (a band: its own rows); which 0 = current, 1 = star
int pe25d_set_tracers(Pe25d *m, int n, const double *c, hipStream_t s, std::string *err);
int pe25d_get_tracers(Pe25d *m, int which, double *c, hipStream_t s, std::string *err);
int pe25d_tracer_count(const Pe25d *m);
int pe25d_set_tracer_scheme(Pe25d *m, int scheme, hipStream_t s, std::string *err);   // gcm_set_tracer_scheme
int pe25d_tracer_scheme(const Pe25d *m);
void pe25d_join_tracers(Pe25d *m, hipStream_t s);   // `s` waits for the last tracer launches on the other streams
void pe25d_follow_tracers(Pe25d *m, hipStream_t s); // a pack / unpack on `s` follows the tracer launches on the second stream
int pe25d_set_band_tracers(Pe25d *m, int n, hipStream_t s, std::string *err);   // gcm_set_band_tracers
int pe25d_set_band_tracer_rows(Pe25d *m, int rows, hipStream_t s, std::string *err);   // gcm_set_band_tracer_rows
int pe25d_band_tracer_rows(const Pe25d *m);   // a band: the depth in force; a single domain: 0
// gcm_tracer_stats: GCM_TRACER_STATS_WORDS doubles per tracer of set `which`, then per q (with_q), own rows only
int pe25d_tracer_stats(Pe25d *m, int which, bool with_q, double *out, int cap, hipStream_t s, std::string *err);
// gcm_set_tracer_forcing (f == nullptr: clear tracer, -1 = all) / gcm_tracer_forced
int pe25d_set_tracer_forcing(Pe25d *m, int tracer, const gcm_tracer_forcing *f, hipStream_t s, std::string *err);
int pe25d_tracer_forced(const Pe25d *m, int tracer);
// gcm_set_tracer_mixing (k == nullptr: clear tracer, -1 = all) / gcm_tracer_mixed
int pe25d_set_tracer_mixing(Pe25d *m, int tracer, const double *k, int nk, hipStream_t s, std::string *err);
int pe25d_tracer_mixed(const Pe25d *m, int tracer);
// gcm_set_tracer_convect / gcm_tracer_convected (pe25d_convect_tracers.hip): the opt-in of a single domain's tracer to the
// mixing in the convective adjustment's blocks; convect_tracer_columns: gcm_convect_tracer_columns (no handle, no device)
int pe25d_set_tracer_convect(Pe25d *m, int tracer, bool on, std::string *err);
int pe25d_tracer_convected(const Pe25d *m, int tracer);
int convect_tracer_columns(int ncol, int L, const double *y, const double *w, const double *dsig, const double *c,
                           double *c_out, int32_t *nblk, std::string *err);
// gcm_tracer_mixing_coeffs (pe25d_tracer_mix.hip; no handle, no device): the tables gcm_set_tracer_mixing's launches take too
int tracer_mixing_coeffs(int L, const double *dsig, const double *k, double dtd, double *lo, double *w, double *g, std::string *err);
void pe25d_timing(Pe25d *m, std::vector<hipEvent_t> *ev, size_t *used);

}  // namespace gcm

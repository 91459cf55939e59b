// GCM_PE25D behind the C ABI: the phases registered behind the dynamics of every step (horizontal diffusion, solar step, Held-Suarez forcing,
// boundary layer, slab ocean, convective adjustment, Betts-Miller convection, moist physics, climatology sample, pressure-level climatology sample, spectra sample, pressure-level maps sample), written down once for gcm_step, gcm_band_run and gcm_end_step, and the entry points that serve GCM_PE25D handles
// only (tracers, step phases and halo buffers, ground and physics, horizontal diffusion, Held-Suarez, boundary layer, convective adjustment, Betts-Miller convection, moist physics, climatology, pressure levels and their heights and maps, spectra, the filter and the taps).
// Host code only: a guard and one forwarding call into the pe25d_* units, through gcm_handle.h and pe25d_kernels.h.
#include <cmath>

#include "gcm_handle.h"
#include "pe25d_phase_geometry.h"
#include "pe25d_stage_geometry.h"

using namespace gcm;

// ------------------------------------------------------------------ the phases of a step
// The order is the model's: the dynamics step, the horizontal diffusion (a single domain's in the walk; a band that has
// opted in: its own rows ahead of the walk, with an exchange of the current state's edge rows between the two --
// pe_band_hdiff_rows), the solar step at the
// current clock, utc += dt, the Held-Suarez forcing,
// the boundary layer, the slab ocean (gcm_set_slab_ocean: pe25d_slab_ocean_on) (on a band with the boundary layer: then
// a third exchange of the edge rows), the convective adjustment, the Betts-Miller
// convection, the moist physics,
// the climatology's sample, the pressure-level climatology's sample, the spectra's sample, the pressure-level maps' sample.  Each launch runs only if its phase is
// registered: the diffusion in pe25d_hdiff_on, the solar step and the forcing in GcmPhases, the boundary layer, the adjustment, the Betts-Miller convection and the moist physics where
// their sums are in place (pe25d_sums_on),
// the four samples in pe25d_sampler_due.  The order is written down in pe_phase_rows and kPeSamples, and in pe_phase_tables for what a
// run prepares ahead of it.

// The registered diffusion's device tables and landing fields for dt; gcm_set_physics: the radiation kernel's tables in
// place before a run queues anything (no-op without physics); then the registered forcing's device tables for dt (none: GCM_OK), the boundary layer's level tables, scratch fields and parameters
// for dt, and the convective adjustment's, the Betts-Miller convection's and the moist physics' level tables and parameters for dt.  Both parts of a
// split walk (gcm_end_step_begin, gcm_end_step_finish) call it: what is in place for dt already is not built again
int pe_phase_tables(gcm_handle *h, int nsteps, double dt) {
    const GcmPhases &ph = h->phases;
    if (nsteps > 0 && pe25d_hdiff_on(h->pe))
        if (int rc = pe25d_hdiff_tables(h->pe, pe25d_hdiff_par(h->pe), dt, h->stream, &h->err)) return rc;
    if (ph.solar)
        if (int rc = pe25d_physics_tables(h->pe, ph.phys.t_lw, ph.phys.t_sw, ph.phys_lat.data(), ph.phys_lon.data(), h->stream, &h->err))
            return rc;
    // gcm_set_gas_radiation: the kernel that takes the solar step's place reads the physics registration's lat and lon
    if (ph.solar && pe25d_gas_radiation_on(h->pe))
        if (int rc = pe25d_gas_radiation_tables(h->pe, pe25d_gas_radiation_par(h->pe), ph.phys_lat.data(), ph.phys_lon.data(), h->stream, &h->err))
            return rc;
    if (nsteps <= 0) return GCM_OK;
    if (ph.held_suarez) {
        gcm_held_suarez hs = ph.hs;
        hs.lat = ph.hs_lat.data();
        if (int rc = pe25d_hs_tables(h->pe, &hs, dt, h->stream, &h->err)) return rc;
    }
    if (pe25d_sums_on(h->pe, kSumsBoundary))
        if (int rc = pe25d_boundary_layer_tables(h->pe, &ph.bl, dt, h->stream, &h->err)) return rc;
    if (pe25d_sums_on(h->pe, kSumsConvect))
        if (int rc = pe25d_convect_tables(h->pe, &ph.cv, dt, &h->err)) return rc;
    if (pe25d_sums_on(h->pe, kSumsBettsMiller))
        if (int rc = pe25d_betts_miller_tables(h->pe, &ph.bm, dt, &h->err)) return rc;
    if (pe25d_sums_on(h->pe, kSumsMoist)) return pe25d_moist_tables(h->pe, &ph.mo, dt, &h->err);
    return GCM_OK;
}

// The registered phases that change the state, over rows [j0, j1) and [jb0, jb1) of state set `set` (-1: the current one)
// on `s`, each launch behind the one before it in stream order.  Every phase but the boundary layer is column-local, so a
// row gets the same bits whichever launch takes it: a single domain's, a band's own rows', a neighbour's ghost rows'.  The
// boundary layer reads neighbouring columns and rows: it takes every row of a single domain, and the own rows of a band
// that has opted in (gcm_set_band_boundary_layer), whose ghost rows are NOT advanced through it -- the caller exchanges
// the current state's edge rows again behind it.  The walk therefore splits there (`which`): kPhasesHead, up to and
// including the boundary layer; kPhasesTail, behind it; kPhasesAll, both, which a band with the boundary layer registered
// refuses.  Two callers:
//  * own: the end of every step, the rows of the handle on its stream (pe_own_row_phases).  The clock advances behind
//    the solar step, and the boundary layer's shf and evap, the convective adjustment's counts and the moist physics'
//    precipitation and evaporation go to the handle's sums (the kernels add rows [0, H) only);
//  * !own: a band's ghost rows as the last exchange delivered them, on the second stream behind the unpack and
//    AHEAD of the ghost rows' column sums and anchors, which read u, v and theta (pe_ghost_row_phases).  The rows are
//    forced locally with the neighbour's own inputs and tables -- theta, p, u, v as delivered, the ground temperature's
//    ghost rows, the latitude of the global row -- hence to the neighbour's own bits.  Their counts and precipitation
//    belong to the neighbour's sums: these launches accumulate nothing, the clock stays, and the boundary layer is
//    skipped (the head's ghost rows are overwritten by the exchange behind it, the tail's arrive with it applied).
// keep_ghosts: the caller forces the ghost rows itself ahead of their column sums and anchors (gcm_band_run), on the
// stream `ghosts` where that is another one than `s` (else null): the boundary layer, which reads v of ghost row -1 and
// all of ghost row H, then waits for that stream's position (the unpack, the ghost rows' solar step and forcing)
static int pe_phase_rows(gcm_handle *h, double dt, int set, int j0, int j1, int jb0, int jb1, bool keep_ghosts, bool own, hipStream_t s,
                         int which, hipStream_t ghosts = nullptr) {
    GcmPhases &ph = h->phases;
    if (which == kPhasesAll && band_boundary_layer_on(h))
        return fail(h, GCM_ERR_STATE, "boundary layer on a latitude band: the phase walk splits at it, with an exchange of the current state between the two parts");
    if (which & kPhasesHead) {
        // gcm_set_hdiff, directly behind the Matsuno step: every row of a single domain.  (A band that has opted in has
        // diffused its own rows ahead of the walk and exchanged its edge rows again: pe_band_hdiff_rows.)  The
        // launch writes u and v, as the forcing's does (pe25d_phase_wrote)
        if (own && h->wrap && pe25d_hdiff_on(h->pe)) {
            if (j0 != 0 || j1 != h->H || jb1 > jb0)
                return fail(h, GCM_ERR_STATE, "horizontal diffusion: the phase walk of a single domain's own rows only");
            if (int rc = pe25d_hdiff_rows(h->pe, set, keep_ghosts, s, &h->err)) return rc;
        }
        if (ph.solar) {
            // no_limits_2_5d.py:229-234 with the physics below full_timestep's early return (:96): the dynamics step, then
            // solar_timestep (:66-75) at the current utc, which changes theta and the ground temperature in place AFTER the
            // post-corrector exchange has left, then utc += dt.  While a gas radiation is registered (gcm_set_gas_radiation)
            // pe25d_solar_rows launches its kernel in place of the grey one, at the same clock and over the same rows
            if (int rc = pe25d_solar_rows(h->pe, set, j0, j1, jb0, jb1, keep_ghosts, dt, ph.phys.utc, ph.phys.albedo, s, &h->err)) return rc;
            if (own) ph.phys.utc += dt;
        }
        // gcm_set_held_suarez, behind the solar step.  The launch writes u and v, which the next stage's chain B reads: it
        // invalidates the fork at the last K4, so that the next step's launches on the second and third stream, which read own
        // rows' u and v, follow this stream's position; and it marks the state's column sums stale, so that behind a ghost-row
        // launch pe25d_prep_ghost_rows leaves them to the next stage (pe25d_phase_wrote)
        if (ph.held_suarez)
            if (int rc = pe25d_hs_rows(h->pe, set, j0, j1, jb0, jb1, keep_ghosts, s, &h->err)) return rc;
        // gcm_set_boundary_layer: u, v, theta and q, behind the forcing: it heats and moistens the lowest level, the
        // adjustment then mixes what became unstable.  The launches write u and v, as the forcing's does.  They take every
        // row of a single domain, the own rows of a band, whatever [j0, j1) says: a single domain's walk is its own rows,
        // all of them, and a band's ghost rows ride in [j0, j1) for the column-local phases only
        if (own && pe25d_sums_on(h->pe, kSumsBoundary)) {
            if (h->wrap && (j0 != 0 || j1 != h->H || jb1 > jb0))
                return fail(h, GCM_ERR_STATE, "boundary layer: the phase walk of a single domain's own rows only");
            if (ghosts && ghosts != s) {                   // (gcm_band_run's own join event: see pe_own_row_phases)
                HIPCHK(h, hipEventRecord(h->band.ev_comm, ghosts));
                HIPCHK(h, hipStreamWaitEvent(s, h->band.ev_comm, 0));
            }
            if (int rc = pe25d_boundary_layer_rows(h->pe, set, keep_ghosts, own, s, &h->err)) return rc;
        }
        // gcm_set_slab_ocean, the end of the head, directly behind the boundary layer: the ground temperature from the
        // flux words the solar step's BUDGET launch and the boundary layer have just stored over the same rows (a phase
        // that is not registered: its words count as zero).  Column-local: the rows as they come, own rows and a band's
        // ghost rows alike, the latter to the neighbour's bits and without sums -- but the own rows only on a band with
        // the boundary layer registered, whose ghost rows have no SH_J and EVAP_KG: their ground temperature arrives
        // with the third exchange, whose message carries it.  The launch writes the ground temperature, the words and
        // the sums, no state field: nothing of the stage's bookkeeping changes
        if (pe25d_slab_ocean_on(h->pe)) {
            const bool bl = pe25d_sums_on(h->pe, kSumsBoundary);
            const bool band_bl = bl && !h->wrap;
            if (own || !band_bl) {
                const int r0 = band_bl ? std::max(j0, 0) : j0, r1 = band_bl ? std::min(j1, h->H) : j1;
                if (int rc = pe25d_slab_ocean_rows(h->pe, r0, r1, band_bl ? 0 : jb0, band_bl ? 0 : jb1, dt, ph.solar, bl, own, s, &h->err))
                    return rc;
            }
        }
    }
    if (!(which & kPhasesTail)) return GCM_OK;
    // gcm_set_convect: theta and q, ahead of the moist physics, which then condenses whatever the mixing left supersaturated
    if (pe25d_sums_on(h->pe, kSumsConvect))
        if (int rc = pe25d_convect_rows(h->pe, set, j0, j1, jb0, jb1, keep_ghosts, own, s, &h->err)) return rc;
    // gcm_set_betts_miller: theta and q, behind the adjustment (which has removed what was unstable against its neutral
    // profile) and ahead of the moist physics, which condenses what the relaxation left supersaturated
    if (pe25d_sums_on(h->pe, kSumsBettsMiller))
        if (int rc = pe25d_betts_miller_rows(h->pe, set, j0, j1, jb0, jb1, keep_ghosts, own, s, &h->err)) return rc;
    // gcm_set_moist: theta and q, the last phase of the step that changes the state
    if (pe25d_sums_on(h->pe, kSumsMoist)) return pe25d_moist_rows(h->pe, set, j0, j1, jb0, jb1, keep_ghosts, own, s, &h->err);
    return GCM_OK;
}

// gcm_band_run with the exchange on the second stream `ax`: the ghost rows' phases, behind an unpack and ahead of
// pe25d_prep_ghost_rows; the band's own rows follow the corrector on the compute stream (pe_own_row_phases).  With the
// boundary layer registered the head follows the corrector's unpack and the tail the third exchange's
int pe_ghost_row_phases(gcm_handle *h, double dt, hipStream_t ax, int which) {
    return pe_phase_rows(h, dt, pe25d_new_state_set(h->pe), -kGhost, 0, h->H, h->H + kGhost, true, false, ax, which);
}

// The samples at the end of a step, in the order they are launched: the climatology's, directly behind it the
// pressure-level climatology's, the spectra's, and the pressure-level maps', the last of the step
struct PeSampleFn { PeSample of; int (*sample)(Pe25d *, hipStream_t, std::string *); };
static constexpr PeSampleFn kPeSamples[] = {{kSampleClimate, pe25d_climate_sample}, {kSamplePlevClimate, pe25d_plev_climate_sample},
                                            {kSampleSpectra, pe25d_spectra_sample}, {kSamplePlevMaps, pe25d_plev_maps_sample}};
static_assert(kPeSamples[kSamplePlevClimate].of == kSamplePlevClimate && kPeSamples[kSampleSpectra].of == kSampleSpectra &&
              kPeSamples[kSamplePlevMaps].of == kSamplePlevMaps, "row i is PeSample i: the entry points index the table by it");

// The end of every step, on the handle's stream: rows [-g, H + g) (phase_ghosts) -- a band's own rows, and the ghost rows
// with them where the exchange was joined into the compute stream.  The compute stream has waited for the edge rows and
// their pack by then (update_interior), so the rows that left are as the corrector made them and the neighbour forces
// them itself.  Callers: gcm_step (g = 0), gcm_band_run, and gcm_end_step, gcm_end_step_begin and gcm_end_step_finish
// for a caller that takes the dynamics step itself.  which: the whole walk, or one of the parts a band with the boundary
// layer registered exchanges between (pe_phase_rows); the samples (kPeSamples) belong to the tail.  tail: the stream whose tail the
// handle's stream joins before a sample, and before a band's boundary layer (gcm_band_run's second stream, where the
// exchange runs and the ghost rows are forced there), else null
int pe_own_row_phases(gcm_handle *h, double dt, int g, bool keep_ghosts, hipStream_t tail, int which) {
    if (int rc = pe_phase_rows(h, dt, -1, -g, h->H + g, 0, 0, keep_ghosts, true, h->stream, which, h->wrap ? nullptr : tail)) return rc;
    if (!(which & kPhasesTail)) return GCM_OK;
    // gcm_set_climate, gcm_set_plev_climate, gcm_set_spectra, gcm_set_plev_maps: a sample of the state the step leaves,
    // behind every phase that changes it.  Each diagnostic counts the step on a counter of its own
    constexpr int N = (int)(sizeof(kPeSamples) / sizeof(kPeSamples[0]));
    bool due[N], any = false;
    for (int i = 0; i < N; ++i) {                          // (every counter counts the step, whatever the others say)
        due[i] = pe25d_sampler_due(h->pe, kPeSamples[i].of);
        any = any || due[i];
    }
    if (!any) return GCM_OK;
    // a band: either sample reads the own rows as the phases above left them on the compute stream, and row -1 of v,
    // the first north ghost row, as the step's last exchange delivered it (the post-corrector exchange and the ghost
    // rows' Held-Suarez launch; with the boundary layer registered the third exchange) -- on the second stream where the
    // exchange runs there.  The compute stream joins that stream's tail first (the
    // unpack, the ghost rows' physics, their column sums), on the steps that sample only, once for all the samples due; the event is
    // gcm_band_run's own join event, which nobody else records between a run's first exchange and its end but the step itself,
    // in stream order
    if (tail) {
        HIPCHK(h, hipEventRecord(h->band.ev_comm, tail));
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->band.ev_comm, 0));
    }
    for (int i = 0; i < N; ++i)
        if (due[i])
            if (int rc = kPeSamples[i].sample(h->pe, h->stream, &h->err)) return rc;
    return GCM_OK;
}

// The registered diffusion of an opted-in band's own rows on the handle's stream, tables in place (pe_phase_tables), from
// the ghost rows -2, -1, H, H + 1 of the selected fields as the corrector's exchange left them.  Behind it the ghost rows
// are stale: the caller exchanges the current state's edge rows again ahead of the phase walk (gcm_band_run:
// band_step_pe_hd; a host-driven step: gcm_end_step_diffuse).  keep_ghosts: as pe_phase_rows
int pe_band_hdiff_rows(gcm_handle *h, bool keep_ghosts) {
    if (!band_hdiff_on(h)) return fail(h, GCM_ERR_STATE, "horizontal diffusion on a latitude band: not registered");
    return pe25d_hdiff_rows(h->pe, -1, keep_ghosts, h->stream, &h->err);
}

// gcm_step of a GCM_PE25D handle (the caller has selected the device)
int pe_step(gcm_handle *h, int nsteps, double dt) {
    if (int rc = pe_phase_tables(h, nsteps, dt)) return rc;
    for (int n = 0; n < nsteps; ++n) {
        if (int rc = pe25d_step(h->pe, dt, h->stream, &h->err)) return rc;
        if (int rc = pe_own_row_phases(h, dt, 0, false, nullptr, kPhasesAll)) return rc;
    }
    pe25d_join_tracers(h->pe, h->stream);             // (the passive tracers' tail on the second stream)
    return GCM_OK;
}

extern "C" {

// ------------------------------------------------------------------ the phases' launch geometry, without launching
int gcm_pe25d_phase_geometry(int phase, int W, int rows, int L, int cus, int elem_bytes, int accumulate, int *out, int nout) {
    return pe25d_phase_geometry(phase, W, rows, L, cus, elem_bytes, accumulate, out, nout);
}

int gcm_pe25d_stage_geometry(int W, int rows, int L, int cus, int elem_bytes, const unsigned *plan, int nplan, int *out, int nout) {
    return pe25d_stage_geometry(W, rows, L, cus, elem_bytes, plan, nplan, out, nout);
}

int gcm_pe25d_stage_plan(gcm_handle *h, int *out, int nout) {
    if (int rc = pe_only(h, "gcm_pe25d_stage_plan")) return rc;
    if (int rc = pe25d_stage_plan(h->pe, out, nout))
        return fail(h, rc, "gcm_pe25d_stage_plan: a null pointer or fewer than GCM_STAGE_PLAN_WORDS words");
    return GCM_OK;
}

int gcm_pe25d_phase_plan(gcm_handle *h, int phase, int rows, int accumulate, int *out, int nout) {
    if (int rc = pe_only(h, "gcm_pe25d_phase_plan")) return rc;
    if (rows == 0) return fail(h, GCM_ERR_ARG, "gcm_pe25d_phase_plan: rows must be 1 or more, or negative for the handle's own");
    if (int rc = pe25d_phase_plan(h->pe, phase, rows, accumulate != 0, out, nout))
        return fail(h, rc, "gcm_pe25d_phase_plan: an unknown phase, a null pointer or fewer than GCM_PHASE_PLAN_WORDS words");
    return GCM_OK;
}

// ------------------------------------------------------------------ the end of a step whose dynamics the caller took itself
// What gcm_band_run queues behind a corrector where the ghost rows ride with the own rows (GCM_BAND_COMM_STREAM=1): the
// tables for dt, then every registered phase over own rows and ghost rows on the handle's stream, the clock, the samples.
// gcm_end_step is the whole walk; gcm_end_step_begin and gcm_end_step_finish are its two parts, for a band with the
// boundary layer registered, which exchanges the current state's edge rows between them.  A band with the horizontal
// diffusion registered has a part of its own ahead of them, gcm_end_step_diffuse, and an exchange behind that
static int end_step_part(gcm_handle *h, double dt, const char *fn, int which) {
    if (int rc = pe_only(h, fn)) return rc;
    if (!std::isfinite(dt)) return fail(h, GCM_ERR_ARG, std::string(fn) + ": dt must be finite");
    if (which == kPhasesAll && band_boundary_layer_on(h))
        return fail(h, GCM_ERR_STATE, std::string(fn) + ": the boundary layer is registered on this band, whose edge rows are exchanged again behind it: "
                                      "call gcm_end_step_begin, exchange the current state's ghost rows, then gcm_end_step_finish");
    const bool hd = band_hdiff_on(h);
    if (hd && which == kPhasesAll)
        return fail(h, GCM_ERR_STATE, std::string(fn) + ": the horizontal diffusion is registered on this band, whose edge rows are exchanged again behind it: "
                                      "call gcm_end_step_diffuse, exchange the current state's ghost rows, then gcm_end_step_begin and gcm_end_step_finish");
    if (hd && (which & kPhasesHead) && !pe25d_band_hdiff_done(h->pe))
        return fail(h, GCM_ERR_STATE, std::string(fn) + ": the horizontal diffusion is registered on this band: call gcm_end_step_diffuse and exchange the "
                                      "current state's ghost rows ahead of gcm_end_step_begin");
    if (int rc = select_device(h)) return rc;
    if (int rc = pe_phase_tables(h, 1, dt)) return rc;
    if (int rc = pe_own_row_phases(h, dt, phase_ghosts(h), false, nullptr, which)) return rc;
    if (hd && (which & kPhasesHead)) pe25d_set_band_hdiff_done(h->pe, false);     // (the next step diffuses again)
    return GCM_OK;
}

// The part of a host-driven step ahead of gcm_end_step_begin: the diffusion of an opted-in, registered band's own rows,
// behind the unpack of the post-corrector exchange.  Every other GCM_PE25D handle: nothing (a single domain's diffusion
// is the head of its walk)
int gcm_end_step_diffuse(gcm_handle *h, double dt) {
    if (int rc = pe_only(h, "gcm_end_step_diffuse")) return rc;
    if (!std::isfinite(dt)) return fail(h, GCM_ERR_ARG, "gcm_end_step_diffuse: dt must be finite");
    if (!band_hdiff_on(h)) return GCM_OK;
    if (int rc = select_device(h)) return rc;
    if (int rc = pe25d_hdiff_tables(h->pe, pe25d_hdiff_par(h->pe), dt, h->stream, &h->err)) return rc;
    if (int rc = pe_band_hdiff_rows(h, false)) return rc;
    pe25d_set_band_hdiff_done(h->pe, true);
    return GCM_OK;
}

int gcm_end_step(gcm_handle *h, double dt) { return end_step_part(h, dt, "gcm_end_step", kPhasesAll); }
int gcm_end_step_begin(gcm_handle *h, double dt) { return end_step_part(h, dt, "gcm_end_step_begin", kPhasesHead); }
int gcm_end_step_finish(gcm_handle *h, double dt) { return end_step_part(h, dt, "gcm_end_step_finish", kPhasesTail); }

// ------------------------------------------------------------------ passive tracers
int gcm_set_tracers(gcm_handle *h, int n, const double *c) {
    if (int rc = pe_on_device(h, "gcm_set_tracers")) return rc;
    const int rc = pe25d_set_tracers(h->pe, n, c, h->stream, &h->err);
    if (rc == GCM_OK && !h->wrap) h->band.primed = false;   // gcm_band_run: the new tracers' ghost rows are not exchanged yet
    return rc;
}

int gcm_set_band_tracers(gcm_handle *h, int n) {
    if (int rc = pe_on_device(h, "gcm_set_band_tracers", true)) return rc;
    return pe25d_set_band_tracers(h->pe, n, h->stream, &h->err);
}

int gcm_set_band_tracer_rows(gcm_handle *h, int rows) {
    if (int rc = pe_on_device(h, "gcm_set_band_tracer_rows", true)) return rc;
    return pe25d_set_band_tracer_rows(h->pe, rows, h->stream, &h->err);
}

int gcm_band_tracer_rows(const gcm_handle *h) {
    if (!h) return GCM_ERR_ARG;
    return h->pe ? pe25d_band_tracer_rows(h->pe) : 0;
}

int gcm_get_tracers(gcm_handle *h, int which, double *c) {
    if (int rc = pe_on_device(h, "gcm_get_tracers")) return rc;
    return pe25d_get_tracers(h->pe, which, c, h->stream, &h->err);
}

int gcm_tracer_stats(gcm_handle *h, int which, int with_q, double *out, int cap) {
    if (!h || !out) return GCM_ERR_ARG;
    if (int rc = pe_on_device(h, "gcm_tracer_stats")) return rc;
    return pe25d_tracer_stats(h->pe, which, with_q != 0, out, cap, h->stream, &h->err);
}

int gcm_set_tracer_forcing(gcm_handle *h, int tracer, const gcm_tracer_forcing *f) {
    if (int rc = pe_on_device(h, "gcm_set_tracer_forcing")) return rc;
    return pe25d_set_tracer_forcing(h->pe, tracer, f, h->stream, &h->err);
}

int gcm_tracer_forced(const gcm_handle *h, int tracer) {
    if (int rc = pe_only(h, "gcm_tracer_forced")) return rc;
    return pe25d_tracer_forced(h->pe, tracer);
}

int gcm_set_tracer_mixing(gcm_handle *h, int tracer, const double *k, int nk) {
    if (int rc = pe_on_device(h, "gcm_set_tracer_mixing")) return rc;
    return pe25d_set_tracer_mixing(h->pe, tracer, k, nk, h->stream, &h->err);
}

int gcm_tracer_mixed(const gcm_handle *h, int tracer) {
    if (int rc = pe_only(h, "gcm_tracer_mixed")) return rc;
    return pe25d_tracer_mixed(h->pe, tracer);
}

int gcm_tracer_mixing_coeffs(int L, const double *dsig, const double *k, double dtd, double *lo, double *w, double *g) {
    return tracer_mixing_coeffs(L, dsig, k, dtd, lo, w, g, &gcm_create_error());
}

// the tracers' convective mixing: the opt-in of a single domain's tracer (a band: refused, not carried yet)
int gcm_set_tracer_convect(gcm_handle *h, int tracer, int on) {
    if (int rc = pe_on_device(h, "gcm_set_tracer_convect")) return rc;
    return pe25d_set_tracer_convect(h->pe, tracer, on != 0, &h->err);
}

int gcm_tracer_convected(const gcm_handle *h, int tracer) {
    if (int rc = pe_only(h, "gcm_tracer_convected")) return rc;
    return pe25d_tracer_convected(h->pe, tracer);
}

int gcm_convect_tracer_columns(int ncol, int L, const double *y, const double *w, const double *dsig, const double *c,
                               double *c_out, int *nblk) {
    return convect_tracer_columns(ncol, L, y, w, dsig, c, c_out, nblk, &gcm_create_error());
}

int gcm_tracer_count(const gcm_handle *h) {
    if (!h) return GCM_ERR_ARG;
    return h->pe ? pe25d_tracer_count(h->pe) : 0;
}

int gcm_set_tracer_scheme(gcm_handle *h, int scheme) {
    if (!h) return GCM_ERR_ARG;
    if (scheme < GCM_TRACER_NONE || scheme > GCM_TRACER_VANLEER)
        return fail(h, GCM_ERR_ARG, "gcm_set_tracer_scheme: scheme must be GCM_TRACER_NONE, _UPWIND or _VANLEER");
    if (int rc = pe_on_device(h, "gcm_set_tracer_scheme")) return rc;
    return pe25d_set_tracer_scheme(h->pe, scheme, h->stream, &h->err);
}

int gcm_tracer_scheme(const gcm_handle *h) {
    if (!h) return GCM_ERR_ARG;
    return h->pe ? pe25d_tracer_scheme(h->pe) : GCM_TRACER_NONE;
}

// ------------------------------------------------------------------ a band's stages driven by the host
int gcm_step_phase(gcm_handle *h, int phase, double dt, void *stream) {
    if (int rc = pe_only(h, "gcm_step_phase", true)) return rc;
    return pe25d_step_phase(h->pe, phase, dt, (hipStream_t)stream, &h->err);
}

int gcm_set_halo_buffers(gcm_handle *h, void *north_send, void *south_send) {
    if (int rc = pe_only(h, "gcm_set_halo_buffers", true)) return rc;
    return pe25d_set_halo_buffers(h->pe, north_send, south_send, h->stream, &h->err);
}

int gcm_wait_edges(gcm_handle *h, void *stream) {
    if (int rc = pe_only(h, "gcm_wait_edges", true)) return rc;
    return pe25d_wait_edges(h->pe, (hipStream_t)stream, &h->err);
}

// ------------------------------------------------------------------ ground temperature and grey physics
int gcm_set_ground(gcm_handle *h, const double *gt) {
    if (!h || !gt) return GCM_ERR_ARG;
    if (int rc = pe_only(h, "gcm_set_ground")) return rc;
    h->band.primed = false;                                // gcm_band_run: the ghost rows of the ground temperature travel again
    return pe25d_ground(h->pe, true, gt, nullptr, h->stream, &h->err);
}

int gcm_get_ground(gcm_handle *h, double *gt) {
    if (!h || !gt) return GCM_ERR_ARG;
    if (int rc = pe_only(h, "gcm_get_ground")) return rc;
    return pe25d_ground(h->pe, false, nullptr, gt, h->stream, &h->err);
}

int gcm_set_physics(gcm_handle *h, const gcm_physics *ph) {
    if (int rc = pe_only(h, "gcm_set_physics")) return rc;
    GcmPhases &p = h->phases;
    if (!ph) {
        p.solar = false;
        return GCM_OK;
    }
    if (!ph->lat || !ph->lon) return fail(h, GCM_ERR_ARG, "gcm_set_physics: lat and lon tables are required");
    // a refused registration changes nothing: the one in place, its clock and its parameters stay
    if (int rc = pe25d_grey_check(h->pe, ph->t_lw, ph->t_sw, ph->albedo, "gcm_set_physics", &h->err)) return rc;
    if (!std::isfinite(ph->utc)) return fail(h, GCM_ERR_ARG, "gcm_set_physics: utc must be finite");
    p.phys = *ph;
    p.phys_lat.assign(ph->lat, ph->lat + h->cfg.global_height);
    p.phys_lon.assign(ph->lon, ph->lon + h->W);
    p.phys.lat = p.phys.lon = nullptr;                     // (the copies above are what is used)
    p.solar = true;
    return GCM_OK;
}

int gcm_get_utc(gcm_handle *h, double *utc) {
    if (!h || !utc) return GCM_ERR_ARG;
    if (!h->phases.solar) return fail(h, GCM_ERR_STATE, "gcm_get_utc: no physics registered (gcm_set_physics)");
    *utc = h->phases.phys.utc;
    return GCM_OK;
}

int gcm_grey_radiation(gcm_handle *h, double utc, double t_lw, double t_sw, double albedo,
                       const double *lat, const double *lon, double *dTdt, double *dt_ground) {
    if (int rc = pe_only(h, "gcm_grey_radiation")) return rc;
    if (int rc = pe25d_grey_check(h->pe, t_lw, t_sw, albedo, "gcm_grey_radiation", &h->err)) return rc;
    if (!std::isfinite(utc)) return fail(h, GCM_ERR_ARG, "gcm_grey_radiation: utc must be finite");
    return pe25d_radiation(h->pe, false, 0.0, utc, t_lw, t_sw, albedo, lat, lon, dTdt, dt_ground,
                           h->stream, &h->err);
}

int gcm_solar_step(gcm_handle *h, double dt, double utc, double t_lw, double t_sw, double albedo,
                   const double *lat, const double *lon) {
    if (int rc = pe_only(h, "gcm_solar_step")) return rc;
    if (int rc = pe25d_grey_check(h->pe, t_lw, t_sw, albedo, "gcm_solar_step", &h->err)) return rc;
    if (!std::isfinite(utc) || !std::isfinite(dt)) return fail(h, GCM_ERR_ARG, "gcm_solar_step: dt and utc must be finite");
    return pe25d_radiation(h->pe, true, dt, utc, t_lw, t_sw, albedo, lat, lon, nullptr, nullptr,
                           h->stream, &h->err);
}

int gcm_grey_radiation_tables(int L, const double *dsig, const double *sig, double t_lw, double t_sw, double *out, int nout) {
    if (L >= 1 && nout < 6 * L) return fail(nullptr, GCM_ERR_ARG, "gcm_grey_radiation_tables: out holds fewer than 6 L doubles");
    return grey_radiation_tables(L, dsig, sig, t_lw, t_sw, out, &gcm_create_error());
}

// ------------------------------------------------------------------ grey radiation by water vapour and CO2
// no ground temperature set: refused in the call itself
int gcm_set_gas_radiation(gcm_handle *h, const gcm_gas_radiation_par *par) {
    if (int rc = pe_on_device(h, "gcm_set_gas_radiation")) return rc;
    return pe25d_set_gas_radiation(h->pe, par, h->stream, &h->err);
}

int gcm_gas_radiation_on(const gcm_handle *h) {
    if (!h) return GCM_ERR_ARG;
    return h->pe && pe25d_gas_radiation_on(h->pe) ? 1 : 0;
}

int gcm_gas_radiation(gcm_handle *h, double utc, const gcm_gas_radiation_par *par, const double *lat, const double *lon,
                      double *dt_ground, double *dt_air, double *olr) {
    if (int rc = pe_on_device(h, "gcm_gas_radiation")) return rc;
    if (int rc = gas_radiation_check(par, "gcm_gas_radiation", &h->err)) return rc;
    if (!std::isfinite(utc)) return fail(h, GCM_ERR_ARG, "gcm_gas_radiation: utc must be finite");
    return pe25d_gas_radiation(h->pe, false, 0.0, utc, par, lat, lon, dt_ground, dt_air, olr, h->stream, &h->err);
}

int gcm_gas_radiation_step(gcm_handle *h, double dt, double utc, const gcm_gas_radiation_par *par, const double *lat, const double *lon) {
    if (int rc = pe_on_device(h, "gcm_gas_radiation_step")) return rc;
    if (int rc = gas_radiation_check(par, "gcm_gas_radiation_step", &h->err)) return rc;
    if (!std::isfinite(utc) || !std::isfinite(dt)) return fail(h, GCM_ERR_ARG, "gcm_gas_radiation_step: dt and utc must be finite");
    return pe25d_gas_radiation(h->pe, true, dt, utc, par, lat, lon, nullptr, nullptr, nullptr, h->stream, &h->err);
}

int gcm_gas_radiation_columns(int ncol, int L, const gcm_gas_radiation_par *par, const double *SC, const double *p, double ptop,
                              const double *sig, const double *dsig, const double *tt, const double *q, const double *gt,
                              double *dt_ground, double *dt_air, double *olr, double *words) {
    return gas_radiation_columns(ncol, L, par, SC, p, ptop, sig, dsig, tt, q, gt, dt_ground, dt_air, olr, words, &gcm_create_error());
}

int gcm_gas_insolation(int kind, int nlat, const double *lat, double declination, double solar_constant, double *out) {
    return gas_insolation(kind, nlat, lat, declination, solar_constant, out, &gcm_create_error());
}

// ------------------------------------------------------------------ horizontal diffusion
// a band opts in to the phase over its own rows and to the exchange per step that goes with it
int gcm_set_band_hdiff(gcm_handle *h, int on) {
    if (int rc = pe_only(h, "gcm_set_band_hdiff", true)) return rc;
    return pe25d_set_band_hdiff(h->pe, on != 0, &h->err);
}

int gcm_band_hdiff(const gcm_handle *h) {
    if (!h) return GCM_ERR_ARG;
    return h->pe && pe25d_band_hdiff(h->pe) ? 1 : 0;
}

// a latitude band that has not opted in, W or H below 4: refused in the call itself
int gcm_set_hdiff(gcm_handle *h, const gcm_hdiff *d) {
    if (int rc = pe_only(h, "gcm_set_hdiff")) return rc;
    if (int rc = select_device(h)) return rc;
    return pe25d_set_hdiff(h->pe, d, h->stream, &h->err);
}

int gcm_hdiff_on(const gcm_handle *h) {
    if (!h) return GCM_ERR_ARG;
    return h->pe && pe25d_hdiff_on(h->pe) ? 1 : 0;
}

int gcm_hdiff_step(gcm_handle *h, double dt, const gcm_hdiff *d) {
    if (int rc = pe_only(h, "gcm_hdiff_step")) return rc;
    if (int rc = hdiff_check(d, "gcm_hdiff_step", &h->err)) return rc;
    if (!std::isfinite(dt)) return fail(h, GCM_ERR_ARG, "gcm_hdiff_step: dt must be finite");
    if (int rc = pe25d_hdiff_fits(h->pe, "gcm_hdiff_step", &h->err)) return rc;
    if (int rc = select_device(h)) return rc;
    // without a registration the call allocates the landing fields itself; the handle keeps them for the next such call,
    // until gcm_set_hdiff(NULL) or gcm_destroy
    // A band that has opted in: its own rows, from current ghost rows; the ghost rows of the selected fields are stale
    // behind the call until the caller's next exchange
    if (int rc = pe25d_hdiff_tables(h->pe, d, dt, h->stream, &h->err)) return rc;
    return pe25d_hdiff_rows(h->pe, -1, false, h->stream, &h->err);
}

int gcm_hdiff_tables(int H, const double *dx_j, const double *dx_h, double dy, const gcm_hdiff *d, double dt, double *out) {
    return hdiff_tables(H, dx_j, dx_h, dy, d, dt, out, &gcm_create_error());
}

int gcm_hdiff_apply(int H, int W, int nlev, const double *tab4, int order, const double *X, double *out) {
    return hdiff_apply(H, W, nlev, tab4, order, X, out, &gcm_create_error());
}

int gcm_hdiff_apply_band(int Hb, int W, int nlev, const double *tab4, int order, const double *X, double *out) {
    return hdiff_apply_band(Hb, W, nlev, tab4, order, X, out, &gcm_create_error());
}

int gcm_hdiff_plan(gcm_handle *h, int *out, int nout) {
    if (int rc = pe_only(h, "gcm_hdiff_plan")) return rc;
    if (int rc = pe25d_hdiff_plan(h->pe, out, nout))
        return fail(h, rc, "gcm_hdiff_plan: a null pointer or fewer than GCM_HDIFF_PLAN_WORDS words");
    return GCM_OK;
}

// ------------------------------------------------------------------ Held-Suarez forcing
int gcm_set_held_suarez(gcm_handle *h, const gcm_held_suarez *hs) {
    if (int rc = pe_only(h, "gcm_set_held_suarez")) return rc;
    GcmPhases &p = h->phases;
    if (!hs) {
        p.held_suarez = false;
        return GCM_OK;
    }
    if (int rc = held_suarez_check(hs, "gcm_set_held_suarez", &h->err)) return rc;
    for (int j = 0; j < h->cfg.global_height; ++j)
        if (!std::isfinite(hs->lat[j])) return fail(h, GCM_ERR_ARG, "gcm_set_held_suarez: lat must be finite");
    p.hs = *hs;
    p.hs_lat.assign(hs->lat, hs->lat + h->cfg.global_height);
    p.hs.lat = nullptr;                                    // (the copy above is what is used)
    p.held_suarez = true;
    return GCM_OK;
}

int gcm_held_suarez_on(const gcm_handle *h) {
    if (!h) return GCM_ERR_ARG;
    return h->pe && h->phases.held_suarez ? 1 : 0;
}

int gcm_held_suarez_step(gcm_handle *h, double dt, const gcm_held_suarez *hs) {
    if (int rc = pe_only(h, "gcm_held_suarez_step")) return rc;
    if (int rc = held_suarez_check(hs, "gcm_held_suarez_step", &h->err)) return rc;
    if (!std::isfinite(dt)) return fail(h, GCM_ERR_ARG, "gcm_held_suarez_step: dt must be finite");
    if (int rc = select_device(h)) return rc;
    if (int rc = pe25d_hs_tables(h->pe, hs, dt, h->stream, &h->err)) return rc;
    // a band: own rows and ghost rows, as gcm_solar_step and gcm_end_step (the ghost rows of the current state must be current)
    const int g = phase_ghosts(h);
    return pe25d_hs_rows(h->pe, -1, -g, h->H + g, 0, 0, false, h->stream, &h->err);
}

int gcm_held_suarez_tables(int L, const double *sig, int nlat, const double *lat, const gcm_held_suarez *hs, double dt,
                           double *fu, double *kt, double *s2, double *c2) {
    return held_suarez_tables(L, sig, nlat, lat, hs, dt, fu, kt, s2, c2, &gcm_create_error());
}

// ------------------------------------------------------------------ surface fluxes and boundary-layer mixing
// a band opts in to the phase over its own rows and to the third exchange per step that goes with it
int gcm_set_band_boundary_layer(gcm_handle *h, int on) {
    if (int rc = pe_only(h, "gcm_set_band_boundary_layer", true)) return rc;
    return pe25d_set_band_boundary_layer(h->pe, on != 0, &h->err);
}

int gcm_band_boundary_layer(const gcm_handle *h) {
    if (!h) return GCM_ERR_ARG;
    return h->pe && pe25d_band_boundary_layer(h->pe) ? 1 : 0;
}

// a latitude band that has not opted in, levels that do not start at the bottom, no ground temperature: refused in the call itself
int gcm_set_boundary_layer(gcm_handle *h, const gcm_boundary_layer *bl) {
    if (int rc = pe_only(h, "gcm_set_boundary_layer")) return rc;
    if (bl) {
        if (int rc = boundary_layer_check(bl, "gcm_set_boundary_layer", &h->err)) return rc;
        if (int rc = pe25d_boundary_layer_fits(h->pe, "gcm_set_boundary_layer", &h->err)) return rc;
    }
    if (int rc = select_device(h)) return rc;
    if (int rc = pe25d_boundary_layer_scratch(h->pe, bl != nullptr, h->stream, &h->err)) return rc;
    if (int rc = pe25d_sums_set(h->pe, kSumsBoundary, bl != nullptr, h->stream, &h->err)) {
        // (a refused call changes nothing: a handle that is not registered keeps no scratch of this call's)
        if (bl && !pe25d_sums_on(h->pe, kSumsBoundary)) {
            std::string ignored;
            (void)pe25d_boundary_layer_scratch(h->pe, false, h->stream, &ignored);
        }
        return rc;
    }
    if (bl) h->phases.bl = *bl;
    return GCM_OK;
}

int gcm_boundary_layer_on(const gcm_handle *h) {
    if (!h) return GCM_ERR_ARG;
    return h->pe && pe25d_sums_on(h->pe, kSumsBoundary) ? 1 : 0;
}

int gcm_boundary_layer_step(gcm_handle *h, double dt, const gcm_boundary_layer *bl) {
    if (int rc = pe_only(h, "gcm_boundary_layer_step")) return rc;
    if (int rc = boundary_layer_check(bl, "gcm_boundary_layer_step", &h->err)) return rc;
    if (!std::isfinite(dt)) return fail(h, GCM_ERR_ARG, "gcm_boundary_layer_step: dt must be finite");
    if (int rc = pe25d_boundary_layer_fits(h->pe, "gcm_boundary_layer_step", &h->err)) return rc;
    if (int rc = select_device(h)) return rc;
    if (int rc = pe25d_boundary_layer_tables(h->pe, bl, dt, h->stream, &h->err)) return rc;
    // the sums of the call go to the registration's accumulators, or nowhere.  Without a registration the call has
    // allocated the scratch fields itself; the handle keeps them for the next such call, until gcm_set_boundary_layer(NULL)
    // or gcm_destroy.  A band that has opted in: its own rows, from current ghost rows; the ghost rows of u, v, theta and q
    // are stale behind the call until the caller's next exchange
    return pe25d_boundary_layer_rows(h->pe, -1, false, pe25d_sums_on(h->pe, kSumsBoundary), h->stream, &h->err);
}

int gcm_get_boundary_layer(gcm_handle *h, double *shf, double *evap, double *seconds, int64_t *nsteps) {
    if (int rc = pe_on_device(h, "gcm_get_boundary_layer")) return rc;
    return pe25d_sums_get(h->pe, kSumsBoundary, shf, evap, seconds, nsteps, h->stream, &h->err);
}

int gcm_put_boundary_layer(gcm_handle *h, const double *shf, const double *evap, double seconds, int64_t nsteps) {
    if (int rc = pe_on_device(h, "gcm_put_boundary_layer")) return rc;
    return pe25d_sums_put(h->pe, kSumsBoundary, shf, evap, seconds, nsteps, h->stream, &h->err);
}

int gcm_boundary_layer_reset(gcm_handle *h) {
    if (int rc = pe_on_device(h, "gcm_boundary_layer_reset")) return rc;
    return pe25d_sums_reset(h->pe, kSumsBoundary, h->stream, &h->err);
}

int gcm_boundary_layer_surface(int n, const gcm_boundary_layer *bl, double ptop, double sig0, const double *uc,
                               const double *vc, const double *theta0, const double *q0, const double *p,
                               double *S, double *z_a, double *cd) {
    return boundary_layer_surface(n, bl, ptop, sig0, uc, vc, theta0, q0, p, S, z_a, cd, &gcm_create_error());
}

int gcm_boundary_layer_column(int ncol, int L, const double *dsig, const double *a, const double *x, const double *target,
                              const double *X, double *X_out, double *X0_surface) {
    return boundary_layer_column(ncol, L, dsig, a, x, target, X, X_out, X0_surface, &gcm_create_error());
}

// ------------------------------------------------------------------ slab mixed-layer ocean
// no ground temperature set: refused in the call itself
int gcm_set_slab_ocean(gcm_handle *h, const gcm_slab_ocean *so, const double *capacity, const double *qflux) {
    if (int rc = pe_on_device(h, "gcm_set_slab_ocean")) return rc;
    return pe25d_set_slab_ocean(h->pe, so, capacity, qflux, h->stream, &h->err);
}

int gcm_slab_ocean_on(const gcm_handle *h) {
    if (!h) return GCM_ERR_ARG;
    return h->pe && pe25d_slab_ocean_on(h->pe) ? 1 : 0;
}

int gcm_slab_ocean_apply(gcm_handle *h, double dt, const gcm_slab_ocean *so, const double *words) {
    if (int rc = pe_on_device(h, "gcm_slab_ocean_apply")) return rc;
    return pe25d_slab_ocean_apply(h->pe, dt, so, words, h->stream, &h->err);
}

int gcm_get_slab_ocean_fluxes(gcm_handle *h, double *words) {
    if (int rc = pe_on_device(h, "gcm_get_slab_ocean_fluxes")) return rc;
    return pe25d_slab_ocean_fluxes(h->pe, words, h->stream, &h->err);
}

int gcm_get_slab_ocean(gcm_handle *h, double *sums, double *seconds, int64_t *nsteps) {
    if (int rc = pe_on_device(h, "gcm_get_slab_ocean")) return rc;
    return pe25d_slab_ocean_get(h->pe, sums, seconds, nsteps, h->stream, &h->err);
}

int gcm_put_slab_ocean(gcm_handle *h, const double *sums, double seconds, int64_t nsteps) {
    if (int rc = pe_on_device(h, "gcm_put_slab_ocean")) return rc;
    return pe25d_slab_ocean_put(h->pe, sums, seconds, nsteps, h->stream, &h->err);
}

int gcm_slab_ocean_reset(gcm_handle *h) {
    if (int rc = pe_on_device(h, "gcm_slab_ocean_reset")) return rc;
    return pe25d_slab_ocean_reset(h->pe, h->stream, &h->err);
}

int gcm_slab_ocean_cells(int n, const gcm_slab_ocean *so, double dt, const double *gt, const double *C, const double *words,
                         const double *Q, double *gt_out, double *E4_out) {
    return slab_ocean_cells(n, so, dt, gt, C, words, Q, gt_out, E4_out, &gcm_create_error());
}

// ------------------------------------------------------------------ convective adjustment
int gcm_set_convect(gcm_handle *h, const gcm_convect *cv) {
    if (int rc = pe_only(h, "gcm_set_convect")) return rc;
    if (cv)
        if (int rc = convect_check(cv, "gcm_set_convect", &h->err)) return rc;
    if (int rc = select_device(h)) return rc;
    if (cv)
        if (int rc = pe25d_convect_fits(h->pe, "gcm_set_convect", &h->err)) return rc;
    if (int rc = pe25d_sums_set(h->pe, kSumsConvect, cv != nullptr, h->stream, &h->err)) return rc;
    if (cv) h->phases.cv = *cv;
    return GCM_OK;
}

int gcm_convect_on(const gcm_handle *h) {
    if (!h) return GCM_ERR_ARG;
    return h->pe && pe25d_sums_on(h->pe, kSumsConvect) ? 1 : 0;
}

int gcm_convect_step(gcm_handle *h, const gcm_convect *cv) {
    if (int rc = pe_only(h, "gcm_convect_step")) return rc;
    if (int rc = convect_check(cv, "gcm_convect_step", &h->err)) return rc;
    if (int rc = select_device(h)) return rc;
    // (the adjustment is instantaneous: the call adds no seconds)
    if (int rc = pe25d_convect_tables(h->pe, cv, 0.0, &h->err)) return rc;
    // a band: own rows and ghost rows, as gcm_moist_step (the ghost rows of the current state must be current); the
    // counts of the call go to the registration's accumulators, or nowhere.  A host that drives the exchange itself ends
    // its steps with gcm_end_step, not with this call
    const int g = phase_ghosts(h);
    return pe25d_convect_rows(h->pe, -1, -g, h->H + g, 0, 0, false, pe25d_sums_on(h->pe, kSumsConvect), h->stream, &h->err);
}

int gcm_get_convect(gcm_handle *h, double *count, double *levels, double *seconds, int64_t *nsteps) {
    if (int rc = pe_on_device(h, "gcm_get_convect")) return rc;
    return pe25d_sums_get(h->pe, kSumsConvect, count, levels, seconds, nsteps, h->stream, &h->err);
}

int gcm_put_convect(gcm_handle *h, const double *count, const double *levels, double seconds, int64_t nsteps) {
    if (int rc = pe_on_device(h, "gcm_put_convect")) return rc;
    return pe25d_sums_put(h->pe, kSumsConvect, count, levels, seconds, nsteps, h->stream, &h->err);
}

int gcm_convect_reset(gcm_handle *h) {
    if (int rc = pe_on_device(h, "gcm_convect_reset")) return rc;
    return pe25d_sums_reset(h->pe, kSumsConvect, h->stream, &h->err);
}

int gcm_convect_columns(int ncol, int L, const double *y, const double *w, const double *q, const double *dsig, int mix_q,
                        double *y_out, double *q_out, int32_t *nblock) {
    return convect_columns(ncol, L, y, w, q, dsig, mix_q, y_out, q_out, nblock, &gcm_create_error());
}

// ------------------------------------------------------------------ Betts-Miller convection
int gcm_set_betts_miller(gcm_handle *h, const gcm_betts_miller *bm) {
    if (int rc = pe_only(h, "gcm_set_betts_miller")) return rc;
    if (bm)
        if (int rc = betts_miller_check(bm, "gcm_set_betts_miller", &h->err)) return rc;
    if (int rc = select_device(h)) return rc;
    if (bm)
        if (int rc = pe25d_betts_miller_fits(h->pe, "gcm_set_betts_miller", &h->err)) return rc;
    if (int rc = pe25d_sums_set(h->pe, kSumsBettsMiller, bm != nullptr, h->stream, &h->err)) return rc;
    if (bm) h->phases.bm = *bm;
    return GCM_OK;
}

int gcm_betts_miller_on(const gcm_handle *h) {
    if (!h) return GCM_ERR_ARG;
    return h->pe && pe25d_sums_on(h->pe, kSumsBettsMiller) ? 1 : 0;
}

int gcm_betts_miller_step(gcm_handle *h, double dt, const gcm_betts_miller *bm) {
    if (int rc = pe_only(h, "gcm_betts_miller_step")) return rc;
    if (int rc = betts_miller_check(bm, "gcm_betts_miller_step", &h->err)) return rc;
    if (!std::isfinite(dt)) return fail(h, GCM_ERR_ARG, "gcm_betts_miller_step: dt must be finite");
    if (int rc = select_device(h)) return rc;
    if (int rc = pe25d_betts_miller_tables(h->pe, bm, dt, &h->err)) return rc;
    // a band: own rows and ghost rows, as gcm_moist_step (the ghost rows of the current state must be current); the sums
    // of the call go to the registration's accumulators, or nowhere.  A host that drives the exchange itself ends its
    // steps with gcm_end_step, not with this call
    const int g = phase_ghosts(h);
    return pe25d_betts_miller_rows(h->pe, -1, -g, h->H + g, 0, 0, false, pe25d_sums_on(h->pe, kSumsBettsMiller), h->stream, &h->err);
}

int gcm_get_betts_miller(gcm_handle *h, double *precip, double *count, double *seconds, int64_t *nsteps) {
    if (int rc = pe_on_device(h, "gcm_get_betts_miller")) return rc;
    return pe25d_sums_get(h->pe, kSumsBettsMiller, precip, count, seconds, nsteps, h->stream, &h->err);
}

int gcm_put_betts_miller(gcm_handle *h, const double *precip, const double *count, double seconds, int64_t nsteps) {
    if (int rc = pe_on_device(h, "gcm_put_betts_miller")) return rc;
    return pe25d_sums_put(h->pe, kSumsBettsMiller, precip, count, seconds, nsteps, h->stream, &h->err);
}

int gcm_betts_miller_reset(gcm_handle *h) {
    if (int rc = pe_on_device(h, "gcm_betts_miller_reset")) return rc;
    return pe25d_sums_reset(h->pe, kSumsBettsMiller, h->stream, &h->err);
}

int gcm_betts_miller_columns(int ncol, int L, const double *p, const double *theta, const double *q, const double *sig,
                             const double *dsig, double ptop, double dt, const gcm_betts_miller *bm, double *theta_out,
                             double *q_out, double *precip, int32_t *kt, int32_t *k_lcl, double *margin) {
    return betts_miller_columns(ncol, L, p, theta, q, sig, dsig, ptop, dt, bm, theta_out, q_out, precip, kt, k_lcl, margin,
                                &gcm_create_error());
}

// ------------------------------------------------------------------ moist physics
int gcm_set_moist(gcm_handle *h, const gcm_moist *mo) {
    if (int rc = pe_only(h, "gcm_set_moist")) return rc;
    if (mo)
        if (int rc = moist_check(mo, "gcm_set_moist", &h->err)) return rc;
    if (int rc = select_device(h)) return rc;
    if (int rc = pe25d_sums_set(h->pe, kSumsMoist, mo != nullptr, h->stream, &h->err)) return rc;
    if (mo) h->phases.mo = *mo;
    return GCM_OK;
}

int gcm_moist_on(const gcm_handle *h) {
    if (!h) return GCM_ERR_ARG;
    return h->pe && pe25d_sums_on(h->pe, kSumsMoist) ? 1 : 0;
}

int gcm_moist_step(gcm_handle *h, double dt, const gcm_moist *mo) {
    if (int rc = pe_only(h, "gcm_moist_step")) return rc;
    if (int rc = moist_check(mo, "gcm_moist_step", &h->err)) return rc;
    if (!std::isfinite(dt)) return fail(h, GCM_ERR_ARG, "gcm_moist_step: dt must be finite");
    if (int rc = select_device(h)) return rc;
    if (int rc = pe25d_moist_tables(h->pe, mo, dt, &h->err)) return rc;
    // a band: own rows and ghost rows, as gcm_held_suarez_step (the ghost rows of the current state must be current);
    // the sums of the call go to the registration's accumulators, or nowhere.  A host that drives the exchange itself
    // ends its steps with gcm_end_step, not with this call
    const int g = phase_ghosts(h);
    return pe25d_moist_rows(h->pe, -1, -g, h->H + g, 0, 0, false, pe25d_sums_on(h->pe, kSumsMoist), h->stream, &h->err);
}

int gcm_get_moist(gcm_handle *h, double *precip, double *evap, double *seconds, int64_t *nsteps) {
    if (int rc = pe_on_device(h, "gcm_get_moist")) return rc;
    return pe25d_sums_get(h->pe, kSumsMoist, precip, evap, seconds, nsteps, h->stream, &h->err);
}

int gcm_put_moist(gcm_handle *h, const double *precip, const double *evap, double seconds, int64_t nsteps) {
    if (int rc = pe_on_device(h, "gcm_put_moist")) return rc;
    return pe25d_sums_put(h->pe, kSumsMoist, precip, evap, seconds, nsteps, h->stream, &h->err);
}

int gcm_moist_reset(gcm_handle *h) {
    if (int rc = pe_on_device(h, "gcm_moist_reset")) return rc;
    return pe25d_sums_reset(h->pe, kSumsMoist, h->stream, &h->err);
}

int gcm_moist_saturation(int n, const double *T, const double *p_lev, double *q_s, double *dq_s, int *can) {
    return moist_saturation_table(n, T, p_lev, q_s, dq_s, can, &gcm_create_error());
}

// ------------------------------------------------------------------ the four sampled diagnostics
// What the entry points of the climatology, the pressure-level climatology, the spectra and the pressure-level maps
// share: the guard and one call into the samplers' routines (pe25d_sampler_*); fn: the entry point's name
static int sampler_set_guard(gcm_handle *h, const char *fn, int every) {
    if (int rc = pe_only(h, fn)) return rc;
    if (every < 0) return fail(h, GCM_ERR_ARG, std::string(fn) + ": every must be >= 0");
    return select_device(h);
}
static int sampler_every(const gcm_handle *h, PeSample of) {
    if (!h) return GCM_ERR_ARG;
    return h->pe ? pe25d_sampler_every(h->pe, of) : 0;
}
// a query that needs the registration (gcm_*_levels, gcm_spectra_mmax)
static int sampler_registered(const gcm_handle *h, PeSample of, const char *fn) {
    if (int rc = pe_only(h, fn)) return rc;
    return pe25d_sampler_registered(h->pe, of, fn, &const_cast<gcm_handle *>(h)->err);
}
static int sampler_sample(gcm_handle *h, PeSample of, const char *fn) {
    if (int rc = pe_on_device(h, fn)) return rc;
    return kPeSamples[of].sample(h->pe, h->stream, &h->err);
}
static int sampler_reset(gcm_handle *h, PeSample of, const char *fn) {
    if (int rc = pe_on_device(h, fn)) return rc;
    return pe25d_sampler_reset(h->pe, of, h->stream, &h->err);
}
static int sampler_get(gcm_handle *h, PeSample of, const char *fn, double *a, double *b, int64_t *nsamples) {
    if (int rc = pe_on_device(h, fn)) return rc;
    return pe25d_sampler_get(h->pe, of, a, b, nsamples, h->stream, &h->err);
}
static int sampler_put(gcm_handle *h, PeSample of, const char *fn, const double *a, const double *b, int64_t nsamples) {
    if (int rc = pe_on_device(h, fn)) return rc;
    return pe25d_sampler_put(h->pe, of, a, b, nsamples, h->stream, &h->err);
}
static int plev_levels(const gcm_handle *h, PeSample of, const char *fn, double *P, int cap) {
    if (int rc = sampler_registered(h, of, fn)) return rc;
    return pe25d_plev_levels(h->pe, of, P, cap);
}

// ------------------------------------------------------------------ zonal wavenumber spectra
int gcm_set_spectra(gcm_handle *h, int every, int mmax) {
    if (int rc = sampler_set_guard(h, "gcm_set_spectra", every)) return rc;
    return pe25d_set_spectra(h->pe, every, mmax, h->stream, &h->err);
}

int gcm_spectra_mmax(const gcm_handle *h) {
    if (int rc = sampler_registered(h, kSampleSpectra, "gcm_spectra_mmax")) return rc;
    return pe25d_spectra_mmax(h->pe);
}

int gcm_spectra_plan(gcm_handle *h, int *out, int nout) {
    if (int rc = pe_only(h, "gcm_spectra_plan")) return rc;
    if (int rc = pe25d_spectra_plan(h->pe, out, nout))
        return fail(h, rc, "gcm_spectra_plan: a null pointer or fewer than GCM_SPEC_PLAN_WORDS words");
    return GCM_OK;
}

int gcm_spectra_every(const gcm_handle *h) { return sampler_every(h, kSampleSpectra); }
int gcm_spectra_sample(gcm_handle *h) { return sampler_sample(h, kSampleSpectra, "gcm_spectra_sample"); }
int gcm_spectra_reset(gcm_handle *h) { return sampler_reset(h, kSampleSpectra, "gcm_spectra_reset"); }
int gcm_get_spectra(gcm_handle *h, double *s, int64_t *nsamples) { return sampler_get(h, kSampleSpectra, "gcm_get_spectra", s, nullptr, nsamples); }
int gcm_put_spectra(gcm_handle *h, const double *s, int64_t nsamples) { return sampler_put(h, kSampleSpectra, "gcm_put_spectra", s, nullptr, nsamples); }

// ------------------------------------------------------------------ pressure levels
int gcm_plev_columns(int ncol, int L, int N, const double *pl, const double *x, const double *P, double *out, int *valid) {
    return plev_columns(ncol, L, N, pl, x, P, out, valid, &gcm_create_error());
}

int gcm_plev_fields(gcm_handle *h, int N, const double *P, double fill, double *out, int32_t *valid) {
    if (int rc = pe_on_device(h, "gcm_plev_fields")) return rc;
    return pe25d_plev_fields(h->pe, N, P, fill, out, valid, h->stream, &h->err);
}

int gcm_set_plev_climate(gcm_handle *h, int every, int N, const double *P) {
    if (int rc = sampler_set_guard(h, "gcm_set_plev_climate", every)) return rc;
    return pe25d_set_plev_climate(h->pe, every, N, P, h->stream, &h->err);
}

int gcm_plev_climate_plan(gcm_handle *h, int *out, int nout) {
    if (int rc = pe_only(h, "gcm_plev_climate_plan")) return rc;
    if (int rc = pe25d_plev_climate_plan(h->pe, out, nout))
        return fail(h, rc, "gcm_plev_climate_plan: a null pointer or fewer than GCM_PLEV_PLAN_WORDS words");
    return GCM_OK;
}

int gcm_plev_climate_every(const gcm_handle *h) { return sampler_every(h, kSamplePlevClimate); }
int gcm_plev_climate_levels(const gcm_handle *h, double *P, int cap) { return plev_levels(h, kSamplePlevClimate, "gcm_plev_climate_levels", P, cap); }
int gcm_plev_climate_sample(gcm_handle *h) { return sampler_sample(h, kSamplePlevClimate, "gcm_plev_climate_sample"); }
int gcm_plev_climate_reset(gcm_handle *h) { return sampler_reset(h, kSamplePlevClimate, "gcm_plev_climate_reset"); }
int gcm_get_plev_climate(gcm_handle *h, double *s, int64_t *nsamples) { return sampler_get(h, kSamplePlevClimate, "gcm_get_plev_climate", s, nullptr, nsamples); }
int gcm_put_plev_climate(gcm_handle *h, const double *s, int64_t nsamples) { return sampler_put(h, kSamplePlevClimate, "gcm_put_plev_climate", s, nullptr, nsamples); }

// ------------------------------------------------------------------ geopotential height on pressure levels, time-mean maps
int gcm_plev_height_columns(int ncol, int L, int N, const double *p, const double *theta, const double *hmG, const double *sig,
                            const double *dsig, const double *sigt, double ptop, const double *P, double *out, int *valid) {
    return plev_height_columns(ncol, L, N, p, theta, hmG, sig, dsig, sigt, ptop, P, out, valid, &gcm_create_error());
}

int gcm_plev_height(gcm_handle *h, int N, const double *P, double fill, double *out, int32_t *valid) {
    if (int rc = pe_on_device(h, "gcm_plev_height")) return rc;
    return pe25d_plev_height(h->pe, N, P, fill, out, valid, h->stream, &h->err);
}

int gcm_set_plev_maps(gcm_handle *h, int every, int N, const double *P) {
    if (int rc = sampler_set_guard(h, "gcm_set_plev_maps", every)) return rc;
    return pe25d_set_plev_maps(h->pe, every, N, P, h->stream, &h->err);
}

int gcm_plev_maps_plan(gcm_handle *h, int *out, int nout) {
    if (int rc = pe_only(h, "gcm_plev_maps_plan")) return rc;
    if (int rc = pe25d_plev_maps_plan(h->pe, out, nout))
        return fail(h, rc, "gcm_plev_maps_plan: a null pointer or fewer than GCM_PLEV_MAP_PLAN_WORDS words");
    return GCM_OK;
}

int gcm_plev_maps_every(const gcm_handle *h) { return sampler_every(h, kSamplePlevMaps); }
int gcm_plev_maps_levels(const gcm_handle *h, double *P, int cap) { return plev_levels(h, kSamplePlevMaps, "gcm_plev_maps_levels", P, cap); }
int gcm_plev_maps_sample(gcm_handle *h) { return sampler_sample(h, kSamplePlevMaps, "gcm_plev_maps_sample"); }
int gcm_plev_maps_reset(gcm_handle *h) { return sampler_reset(h, kSamplePlevMaps, "gcm_plev_maps_reset"); }
int gcm_get_plev_maps(gcm_handle *h, double *s, double *s2, int64_t *nsamples) { return sampler_get(h, kSamplePlevMaps, "gcm_get_plev_maps", s, s2, nsamples); }
int gcm_put_plev_maps(gcm_handle *h, const double *s, const double *s2, int64_t nsamples) { return sampler_put(h, kSamplePlevMaps, "gcm_put_plev_maps", s, s2, nsamples); }

// ------------------------------------------------------------------ zonal-mean climatology
int gcm_set_climate(gcm_handle *h, int every) {
    if (int rc = sampler_set_guard(h, "gcm_set_climate", every)) return rc;
    return pe25d_set_climate(h->pe, every, h->stream, &h->err);
}

int gcm_climate_every(const gcm_handle *h) { return sampler_every(h, kSampleClimate); }
int gcm_climate_sample(gcm_handle *h) { return sampler_sample(h, kSampleClimate, "gcm_climate_sample"); }
int gcm_climate_reset(gcm_handle *h) { return sampler_reset(h, kSampleClimate, "gcm_climate_reset"); }
int gcm_get_climate(gcm_handle *h, double *m3, double *m2, int64_t *nsamples) { return sampler_get(h, kSampleClimate, "gcm_get_climate", m3, m2, nsamples); }
int gcm_put_climate(gcm_handle *h, const double *m3, const double *m2, int64_t nsamples) { return sampler_put(h, kSampleClimate, "gcm_put_climate", m3, m2, nsamples); }

// ------------------------------------------------------------------ the filter of a field, the stage's intermediates
int gcm_polar_filter(gcm_handle *h, int nlev, const double *in, double *out) {
    if (!h || !in || !out) return GCM_ERR_ARG;
    if (int rc = pe_on_device(h, "gcm_polar_filter")) return rc;
    return pe25d_filter_field(h->pe, nlev, in, out, h->stream, &h->err);
}

int gcm_get_intermediate(gcm_handle *h, int kind, double *out) {
    if (!h || !out) return GCM_ERR_ARG;
    if (int rc = pe_on_device(h, "gcm_get_intermediate")) return rc;
    return pe25d_intermediate(h->pe, kind, out, h->stream, &h->err);
}

}  // extern "C"

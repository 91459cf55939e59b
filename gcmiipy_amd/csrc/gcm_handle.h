// The handle behind the C ABI of include/gcmcore.h, private to gcmcore.hip (create / destroy, state transfer, the 2-D
// step, ghost rows, timing), gcm_band.hip (gcm_band_run: the exchange the library posts itself), gcm_diag.hip (the
// reductions) and gcm_pe.hip (the GCM_PE25D-only entry points and the phases of a GCM_PE25D step): the struct, the few
// helpers more than one of them uses, and what the others reach in gcmcore.hip and gcm_pe.hip.
#pragma once
#include "../../include/gcmcore.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "pe25d_kernels.h"
#include "sw2d_kernels.h"

// gcm_band_run: the exchange the library posts itself (gcm_band.hip)
struct GcmBandExchange {
    gcm_exchange xch{};
    bool set = false, primed = false;
    bool inflight = false;                     // an exchange posted, its unpack still to come
    bool overlap = false;                      // deep-halo bands: hide the exchange behind interior rows (gcm_set_band_overlap)
    hipEvent_t ev_pack = nullptr, ev_comm = nullptr;
    bool join_pending = false;                 // GCM_PE25D: work on the second stream not yet joined
    bool on_comm = false;                      // GCM_BAND_COMM_STREAM=1 at gcm_set_exchange: exchange on the comm stream, a join per stage
};

// per-launch timing of the dominant kernel (gcm_time_steps second pass)
struct GcmTiming {
    bool on = false;
    std::vector<hipEvent_t> ev, region;        // region: start / end of gcm_time_steps' timed region
    size_t used = 0;
};

// GCM_PE25D: the phases registered behind the dynamics of every step (gcm_pe.hip runs them; the climatology's
// registration is Pe25d's own, and so are the convective adjustment's, the Betts-Miller convection's and the moist physics': pe25d_sums_on -- mo, cv, bm
// and bl are the parameters their steps run with).  The records' table pointers are null: the vectors are the copies that are used
struct GcmPhases {
    bool solar = false;                        // gcm_set_physics: solar_timestep as the second phase of every step
    bool held_suarez = false;                  // gcm_set_held_suarez: the forcing behind the solar step
    gcm_physics phys{};                        // phys.utc is the clock: it advances by dt behind every solar step
    gcm_held_suarez hs{};
    gcm_moist mo{};
    gcm_convect cv{};
    gcm_betts_miller bm{};
    gcm_boundary_layer bl{};
    std::vector<double> phys_lat, phys_lon, hs_lat;
};

struct gcm_handle {
    gcm_config cfg{};
    int W = 0, H = 0, L = 1;
    bool wrap = true;  // nranks == 1: periodic rows by index arithmetic
    hipStream_t stream = nullptr;
    std::string err;
    std::vector<void *> allocs;

    // 2-D models: per-field arrays of (H + 2*kGhost) rows; pointers address interior row 0.  An fp32 handle
    // (GCM_SW2D / GCM_SW2D_TEMP with dtype GCM_F32) keeps float arrays at these addresses: esz = 4, and every
    // offset into them goes through at() (elements of esz bytes)
    double *cur[GCM_NFIELDS] = {}, *nxt[GCM_NFIELDS] = {}, *star[GCM_NFIELDS] = {};
    double *geo = nullptr, *irho = nullptr, *sst = nullptr, *qtmp = nullptr;
    bool has[GCM_NFIELDS] = {};
    double *exner_tab = nullptr;
    int G = gcm::kGhost;     // ghost rows per side = 2 * steps between exchanges (2-D bands)
    int since_exchange = 0;  // steps taken on the current ghost rows
    bool ghosts_current = false;  // 2-D bands: the current state's ghost rows were filled after its last step
    bool star_valid = false;
    bool launch_refused = false;      // hipLaunchKernel of the fused step returned an error (reported by launch_status)
    hipStream_t comm = nullptr;       // gcm_comm_stream: owned, created on first request
    double *snap[GCM_NFIELDS] = {};   // gcm_snapshot: device copy of the state, ghost rows included
    int snap_since_exchange = 0;
    int variant = GCM_VARIANT_FUSED;
    int rows_per_band = 32;
    int M = 1;              // ensemble members (2-D models, single band)
    long mstride = 0;       // elements from one member's slab to the next: (H + 2G) W, rounded up to 256 B if M > 1
    bool f32 = false;       // 2-D models: float storage and arithmetic (gcm_config.dtype == GCM_F32)
    int esz = 8;            // bytes per element of the 2-D state
    int cols = 1;           // fused kernel: columns per lane (2: fp32 with an even width, 120-column strips)
    int depth_pin = 0;      // GCM_SW2D_DEPTH at gcm_create (float64 GCM_SW2D_TEMP only): 1 or 3 pins the fused form's depth, 0: none
    int pair_pin = -1;      // GCM_SW2D_PAIR at gcm_create (float64 GCM_SW2D_TEMP only): 0 or 1 pins the wave pair off or on, -1: none
    int pair_rows = 0;      // the wave pair's own band length (sw2d_pair_rows_per_band); 0: a handle the pair never serves
    double *staging = nullptr;  // fp32 handles: float64 staging buffer of state transfers, staging_members members
    int staging_members = 0;

    // diagnostics scratch
    double *diag_dev = nullptr;
    static constexpr int kDiagBlocks = 512;

    GcmTiming time;
    gcm::Pe25d *pe = nullptr;  // GCM_PE25D state (pe25d_kernels.h)
    GcmBandExchange band;
    GcmPhases phases;
};

#define HIPCHK(h, call)                                                                    \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) {                                                            \
            char b_[512];                                                                  \
            snprintf(b_, sizeof b_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                     __FILE__, __LINE__);                                                  \
            (h)->err = b_;                                                                 \
            return GCM_ERR_HIP;                                                            \
        }                                                                                  \
    } while (0)

// (what follows is shared by the library's own units only: none of it is exported)
#pragma GCC visibility push(hidden)

std::string &gcm_create_error();   // the calling thread's message of an entry point that has no handle (gcm_last_error(NULL))

inline int fail(gcm_handle *h, int code, const std::string &msg) {
    if (h) h->err = msg;
    else gcm_create_error() = msg;
    return code;
}

// p + n elements of the handle's 2-D state (esz bytes each)
inline double *at(const gcm_handle *h, double *p, long n) { return (double *)((char *)p + n * h->esz); }

// elements of one 2-D field: all members, ghost rows included
inline size_t all_members_elems(const gcm_handle *h) {
    return (size_t)(h->M - 1) * h->mstride + (size_t)(h->H + 2 * h->G) * h->W;
}

// diagnostics: workgroups per member of the reduction kernels (one member: gcm_handle::kDiagBlocks)
inline int diag_blocks_per_member(const gcm_handle *h) { return std::max(8, gcm_handle::kDiagBlocks / h->M); }

// the calls that follow go to the handle's device
inline int select_device(gcm_handle *h) {
    if (h->cfg.device >= 0) HIPCHK(h, hipSetDevice(h->cfg.device));
    return GCM_OK;
}

// the guards of the entry points that serve one kind of handle only; fn is the message's prefix
inline int pe_only(const gcm_handle *h, const char *fn, bool bands = false) {
    if (!h) return GCM_ERR_ARG;
    if (h->pe) return GCM_OK;
    return fail(const_cast<gcm_handle *>(h), GCM_ERR_UNSUPPORTED, std::string(fn) + (bands ? ": GCM_PE25D latitude bands only" : ": GCM_PE25D only"));
}
// ... and whose next calls go to the handle's device
inline int pe_on_device(gcm_handle *h, const char *fn, bool bands = false) {
    if (int rc = pe_only(h, fn, bands)) return rc;
    return select_device(h);
}
inline int band_only(gcm_handle *h, const char *fn) {
    if (!h) return GCM_ERR_ARG;
    if (h->wrap) return fail(h, GCM_ERR_STATE, std::string(fn) + ": handle is not a latitude band");
    return GCM_OK;
}

// gcmcore.hip, for gcm_band.hip (the ghost rows go through gcm_halo_pack2 / gcm_halo_unpack2); defined among the entry points
extern "C" void step_rows(gcm_handle *h, double dt, int j0, int j1, hipStream_t s);
extern "C" void swap_state(gcm_handle *h);
extern "C" int launch_status(gcm_handle *h);

// gcm_pe.hip, for gcm_step, gcm_band_run and gcm_end_step: the phases of a GCM_PE25D step (solar step, utc += dt, Held-Suarez, boundary layer, convective adjustment, Betts-Miller convection, moist physics, the climatology's sample, the pressure-level climatology's sample, the spectra's sample), each
// launched only if it is registered -- their tables before a run, a band's ghost rows on its second stream `ax` behind a
// corrector's unpack, and the end of every step on the handle's stream over rows [-g, H + g), which joins `tail` before a sample
// The walk splits at the boundary layer (`which`): a band that carries it exchanges the current state's edge rows between
// kPhasesHead (solar step, clock, Held-Suarez, boundary layer over the own rows) and kPhasesTail (convective adjustment,
// Betts-Miller convection, moist physics, sample); everybody else walks kPhasesAll
enum { kPhasesHead = 1, kPhasesTail = 2, kPhasesAll = 3 };
extern "C" int pe_step(gcm_handle *h, int nsteps, double dt);        // gcm_step of a GCM_PE25D handle
extern "C" int pe_phase_tables(gcm_handle *h, int nsteps, double dt);
extern "C" int pe_ghost_row_phases(gcm_handle *h, double dt, hipStream_t ax, int which);
extern "C" int pe_own_row_phases(gcm_handle *h, double dt, int g, bool keep_ghosts, hipStream_t tail, int which);
// a band with the boundary layer registered (which takes the opt-in, gcm_set_band_boundary_layer): three exchanges per step
inline bool band_boundary_layer_on(const gcm_handle *h) { return h->pe && !h->wrap && gcm::pe25d_sums_on(h->pe, gcm::kSumsBoundary); }
// a band with the horizontal diffusion registered (which takes the opt-in, gcm_set_band_hdiff): its own rows are diffused
// behind the corrector's unpack and the current state's edge rows exchanged once more ahead of the phase walk
inline bool band_hdiff_on(const gcm_handle *h) { return h->pe && !h->wrap && gcm::pe25d_hdiff_on(h->pe); }
extern "C" int pe_band_hdiff_rows(gcm_handle *h, bool keep_ghosts);
// ghost rows a side that a phase's launch on the handle's stream takes with the own rows: a band's, unless they are
// forced apart on the second stream (pe_ghost_row_phases)
inline int phase_ghosts(const gcm_handle *h, bool apart = false) { return h->wrap || apart ? 0 : gcm::kGhost; }

#pragma GCC visibility pop

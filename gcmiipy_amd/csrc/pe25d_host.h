// Host side of GCM_PE25D, private to its five host units: the handle and the few helpers they share.
//   pe25d_state.hip    the handle's life cycle and data movement: create / destroy (and the one reader of the GCM_PE_*
//                      switches), the streams, set / get and the layout transposes, halo buffers and segments; what the
//                      phases behind the dynamics share: their column sums, the level table, pe25d_phase_wrote; what the
//                      four sampled diagnostics share: every / due / reset / get / put / free of a PeSampler
//   pe25d_kernels.hip  the stage orchestration (half_t and its steps) and the column kernels K2 it launches
//   pe25d_physics.hip  grey radiation and the ground temperature
//   pe25d_diag.hip     diagnostics and taps: gcm_stats, the polar filter of a field, the stage's intermediates
//   pe25d_tracers.hip  the passive tracers' host side
//   pe25d_held_suarez.hip  the Held-Suarez forcing: its table routine, its kernel and its launches
//   pe25d_climate.hip  the zonal-mean climatology: its kernel, its sums and their way to the host and back
//   pe25d_spectra.hip  the zonal wavenumber spectra: their kernel, their sums and their way to the host and back
//   pe25d_plev.hip     pressure levels: the column rule's host build, the map and sample kernels, the sample's sums
//   pe25d_plev_height.hip  geopotential height on pressure levels: the rule's host build, the kernel, the maps' sums
//   pe25d_moist.hip    moist physics: the saturation routine, the kernel and its launches
//   pe25d_convect.hip  convective adjustment: the pooling routine, the kernel and its launches
//   pe25d_betts_miller.hip  Betts-Miller convection: the column routines, the kernel and its launches
//   pe25d_convect_tracers.hip  the tracers' convective mixing in the adjustment's blocks: the kernel, its launch, the opt-ins
//   pe25d_boundary_layer.hip  surface fluxes and boundary-layer mixing: the routines, the two kernels and their launches
//   pe25d_slab_ocean.hip  the slab mixed-layer ocean: the cell routine's probe, the kernel, its launches, words and sums
//   pe25d_gas_radiation.hip  grey radiation by water vapour and CO2: the column routine's probe, the kernel, its tables and launches
//   pe25d_hdiff.hip    horizontal diffusion: the table and cell routines, the tile kernel, its launch and landing fields
// A kernel is instantiated, launched and given its LDS attribute in one unit only (a second unit would get a host stub
// of its own, which an attribute set through the first does not reach).  gcmcore.hip, gcm_band.hip, gcm_diag.hip and
// gcm_pe.hip see pe25d_kernels.h only; of these, gcm_pe.hip alone launches the phases behind a step (pe25d_solar_rows,
// pe25d_hdiff_rows, pe25d_hs_rows, pe25d_boundary_layer_rows, pe25d_convect_rows, pe25d_betts_miller_rows, pe25d_moist_rows, and behind
// pe25d_sampler_due the four samples: pe25d_climate_sample, pe25d_plev_climate_sample, pe25d_spectra_sample,
// pe25d_plev_maps_sample).
#pragma once
#include "pe25d_kernels.h"

#include "pe25d_dev.h"

namespace gcm {

// Device buffers in the handle's real type T (fp64, or fp32 for the tolerance sweep).
template <typename T>
struct PeBufs {
    using T2 = typename Vec2<T>::type;
    // state sets: 0/1 ping-pong (cur = set[cur_i]), 2 = star.  [f] p,u,v,t,q; interior pointers
    T *st[3][GCM_NFIELDS] = {};
    T *spu = nullptr, *phi = nullptr, *pgfu = nullptr, *pit = nullptr, *pn = nullptr;
    T *cs[3][2] = {};                           // per state set: sum_k dsig[k] u[k], sum_k dsig[k] v[k] (2-D)
    T *part = nullptr;                          // (kMaxSeg - 1) slabs like pit
    T *cor_u = nullptr, *cor_v = nullptr;
    T *inv_dxj = nullptr, *inv_dxh = nullptr, *sig = nullptr, *dsig = nullptr, *inv_dsig = nullptr,
      *sigb = nullptr, *sigt = nullptr, *heightmap = nullptr, *smul = nullptr;
    T2 *tw = nullptr;
};

// What the handle holds for its passive tracers; pending, ev_tr, ev_tr_int and int_* are the stream protocol, pe25d_tracers.hip's alone
struct PeTracers {
    // passive tracers (gcm_set_tracers; a band: gcm_set_band_tracers first): 2 x n fields of (H + 2 tr_ghost(m)) x L x W
    // in T, device layout [j][k][i] -- the current set (n fields), then the star set; a band's fields carry `rows`
    // ghost rows a side (gcm_set_band_tracer_rows: 1, or the 2 the van Leer scheme reads), addressed from interior row
    // 0.  The tracer kernel runs on chain B
    // (see stage_tracers); ev_tr, recorded on `aux` behind the last tracer launch, is how the caller's stream joins that tail
    int n = 0;
    void *buf = nullptr;
    int rows = 1;                               // gcm_set_band_tracer_rows: a band's tracer ghost rows per side (see tr_ghost)
    int scheme = GCM_TRACER_NONE;               // gcm_set_tracer_scheme: the face values of the tracers' fluxes
    bool star = false;                          // the star set holds the tracers of a predictor
    bool pending = false;                       // a tracer launch on `aux` that the caller's stream has not joined
    hipEvent_t ev_tr = nullptr;
    // a band's split stage (modes 1 + 2) runs the tracers' interior rows on the third stream (see stage_tracers): ev_tr_int
    // follows that launch; the next stage's chain B waits for it (int_wait), the caller's stream joins it (int_join)
    hipEvent_t ev_tr_int = nullptr;
    hipStream_t int_stream = nullptr;
    bool int_wait = false, int_join = false;
    // forcing of the tracers (gcm_set_tracer_forcing, pe25d_tracer_force.h): per tracer the record and its fields on
    // the device, own rows in the tracers' layout [j][k][i], placed within 16 bytes like the tracer's own row 0 (the
    // wide path of the kernel); n_forced of them are registered.  Applied behind the corrector's launches (launch_tracers)
    struct Force {
        bool on = false;
        double source = 0.0, decay = 0.0, pin_value = 0.0;
        void *emis_alloc = nullptr, *mask_alloc = nullptr;     // what hipMalloc gave
        void *emis = nullptr;                                  // own row 0, in T
        unsigned char *mask = nullptr;                         // own row 0
    };
    Force force[GCM_MAX_TRACERS];
    int n_forced = 0;
    // implicit vertical mixing of the tracers (gcm_set_tracer_mixing, pe25d_tracer_mix.h): per tracer the float64
    // profile K [L - 1] (empty: not mixed); n_mixed of them are registered.  The kernel's tables -- lo, w, g [L] in the
    // handle's real type per mixed tracer, in tracer order -- are built for one dt (dt_built, valid with `built`) and
    // built again when a stage comes with another, into the other of the two device buffers (an earlier launch on
    // another stream may still read the first); ev_tab follows the upload on tab_stream, and the other streams of a
    // stage wait for it once (waited).  Applied behind the corrector's launches, ahead of the forcing (launch_tracers)
    struct Mix {
        std::vector<double> k[GCM_MAX_TRACERS];
        int n_mixed = 0;
        void *tab[2] = {nullptr, nullptr};
        int cur = 0;
        bool built = false;
        double dt_built = 0.0;
        hipEvent_t ev_tab = nullptr;
        hipStream_t tab_stream = nullptr;
        hipStream_t waited[4] = {};
        int n_waited = 0;
    };
    Mix mix;
    // convective mixing of the tracers (gcm_set_tracer_convect, pe25d_convect_tracers.hip): per tracer the opt-in,
    // n_convect of them; convect_lds: the kernel's dynamic LDS at the handle's L, 0: its attribute is not set yet
    bool convect[GCM_MAX_TRACERS] = {};
    int n_convect = 0;
    size_t convect_lds = 0;
    double *stats_dev = nullptr;               // gcm_tracer_stats: float64 dsig [L], the records, then the workgroups' partials
};

// Held-Suarez forcing (pe25d_held_suarez.hip): the device tables of the last (parameters, lat, dt) a launch was asked
// for -- `key`, compared on every step, so that they are built and uploaded again only when one of them changes
struct PeHeldSuarez {
    double *tab = nullptr;                      // device: 4 x [L] level tables, 2 x [Hg], 2 x [L][Hg]
    std::vector<double> key;                    // the eight parameters, dt, lat [Hg]
    double par[5] = {};                         // T_min, T_0, dT_y, dtheta_z, (free): what the kernel takes by value
};

// A sampled diagnostic (gcm_set_climate, gcm_set_plev_climate, gcm_set_spectra, gcm_set_plev_maps): float64 sums on the
// device behind `head` words of tables, one or two blocks of them, and the two counters.  One set of routines serves the
// four (pe25d_sampler_*, pe25d_state.hip); kPeSamplerWords, in the order of PeSample, holds the words in which their
// messages differ.  A unit's own part is its pe25d_set_* (which fills head and words), its *_sample and its *_plan
struct PeSampler {
    double *buf = nullptr;                      // device: head words, then the sums: words[0] of them, then words[1]
    int every = 0;                              // a sample every so many steps; 0: not registered
    long long steps = 0;                        // steps taken by gcm_step / gcm_band_run since the registration
    long long n = 0;                            // samples in the sums
    size_t head = 0;                            // float64 words ahead of the sums
    size_t words[2] = {0, 0};                   // the sizes of the sum blocks; words[1] = 0: one block
};
struct PeSamplerWords { const char *name, *what, *a, *b; };   // gcm_set_<name>, "no <what> registered", the sum arguments (b null: one)
constexpr PeSamplerWords kPeSamplerWords[] = {{"climate", "climatology", "m3", "m2"},                      // kSampleClimate
                                              {"plev_climate", "pressure-level climatology", "s", nullptr},  // kSamplePlevClimate
                                              {"spectra", "spectra", "s", nullptr},                          // kSampleSpectra
                                              {"plev_maps", "pressure-level maps", "s", "s2"}};              // kSamplePlevMaps
// buf of the zonal-mean climatology (pe25d_climate.hip; a PeSampler and nothing else):
//   sig [L], m3 [GCM_CLIM_WORDS3][L][H], m2 [GCM_CLIM_WORDS2][H]
// The two on pressure levels: the registered targets' host copy (its size is N) beside the sampler.  buf of the zonal-mean
// climatology (pe25d_plev.hip): P [N], s [GCM_PLEV_WORDS][N][H]; of the time-mean maps (pe25d_plev_height.hip): P [N],
// s [GCM_PLEV_MAP_WORDS][N][H][W], s2 [GCM_PLEV_MAP_WORDS2][H][W]
struct PePlev : PeSampler {
    std::vector<double> P;                      // the registered targets, Pa; meaningful while every > 0
};
// Zonal wavenumber spectra (pe25d_spectra.hip): buf holds tw [W] double2, sig [L], s [GCM_SPEC_WORDS][L][H][mmax + 1]
struct PeSpectra : PeSampler {
    int mmax = 0;                               // the highest wavenumber in the sums; meaningful while every > 0
};

// The float64 column sums of a phase that runs behind the dynamics, with their two counters: two [H][W] fields of the
// band's own rows.  One set of routines serves every such phase (pe25d_sums_*, pe25d_state.hip); kPeSumsWords holds the
// words in which their messages differ
struct PeColumnSums {
    double *acc = nullptr;                      // device: the first field [H][W], then the second; non-null: registered
    double seconds = 0.0;                       // sum of dt over the applications in the sums
    long long n = 0;                            // applications in the sums
};
struct PeSumsWords { const char *name, *what, *a, *b; };   // gcm_set_<name>, "no <what> registered", the two fields
constexpr PeSumsWords kPeSumsWords[] = {{"convect", "convective adjustment", "count", "levels"},     // kSumsConvect
                                        {"moist", "moist physics", "precip", "evap"},                // kSumsMoist
                                        {"boundary_layer", "boundary layer", "shf", "evap"},         // kSumsBoundary
                                        {"betts_miller", "Betts-Miller convection", "precip", "count"}};   // kSumsBettsMiller
// an accumulating launch went out: one application of dt
inline void sums_count(PeColumnSums &z, double dt) { z.seconds += dt; ++z.n; }

// Moist physics (pe25d_moist.hip, gcm_set_moist): the sums (precip, evap) and the parameters of the launches that follow
// (pe25d_moist_tables)
struct PeMoist {
    PeColumnSums sums;
    int kb = 0;                                 // the level with the largest sig: the one the surface moistens
    double lc = 0.0, x = 0.0, rh_s = 0.0, dt = 0.0;   // Lv / Cp, dt / tau_e (0: no evaporation), rh_s, dt
};

// Convective adjustment (pe25d_convect.hip, gcm_set_convect): the sums (count, levels; their seconds count the registered
// steps' dt only) and the parameters of the launches that follow (pe25d_convect_tables)
struct PeConvect {
    PeColumnSums sums;
    size_t lds_bytes = 0;                       // the kernel's dynamic LDS at the handle's L; 0: not checked against the device yet
    double kappa_c = 0.0, dt = 0.0;             // the neutral profile (0: dry); what an accumulating launch adds to seconds
    int mix_q = 0;
};

// Betts-Miller convection (pe25d_betts_miller.hip, gcm_set_betts_miller): the sums (precip, count) and the parameters of
// the launches that follow (pe25d_betts_miller_tables)
struct PeBettsMiller {
    PeColumnSums sums;
    size_t lds_bytes = 0;                       // the kernel's dynamic LDS at the handle's L; 0: not checked against the handle and the device yet
    double lc = 0.0, r = 0.0, rh_bm = 0.0, dt = 0.0;   // Lv / Cp, x / (1 + x) with x = dt / tau, rh_bm, dt
    int nsub = 0;
};

// Surface fluxes and boundary-layer mixing (pe25d_boundary_layer.hip, gcm_set_boundary_layer): the sums (shf, evap), the
// float64 scratch fields the two launches hand each other and the parameters of the launches that follow
// (pe25d_boundary_layer_tables)
struct PeBoundary {
    PeColumnSums sums;
    bool band = false;                          // gcm_set_band_boundary_layer: a band takes the phase over its own rows
    double *scratch = nullptr;                  // device: cd [R][W], r [R][W], e [R][L-1][W], R = H (a band: H + 1); L > 40: four park fields [H][L][W]
    gcm_boundary_layer par{};
    double dt = 0.0;
};

// Slab mixed-layer ocean (pe25d_slab_ocean.hip, gcm_set_slab_ocean): the registration and its parameters, the float64
// flux words the radiation's BUDGET launch and the boundary layer store while it is registered, the optional fields and
// the sums with their two counters.  Everything is allocated by the registration (the words also by gcm_slab_ocean_apply)
struct PeSlab {
    bool on = false;                            // gcm_set_slab_ocean: registered
    gcm_slab_ocean par{};
    double *words = nullptr;                    // device: GCM_SLAB_WORDS fields [H + 2 kGhost][W], from ghost row -kGhost
    double *sums = nullptr;                     // device: GCM_SLAB_SUMS fields [H][W]
    double *cap = nullptr, *qflux = nullptr;    // device: [H][W], or null (the scalar heat capacity; no heat flux)
    double seconds = 0.0;                       // sum of dt over the applications in the sums
    long long n = 0;                            // applications in the sums
};

// Grey radiation by water vapour and CO2 (pe25d_gas_radiation.hip, gcm_set_gas_radiation): the registration and its
// parameters, the insolation of every global row for the last ("uniform" | "daily", declination, solar_constant) a launch
// was asked for -- `key`, compared on every step -- and the diagnostic form's float64 dt_ground and olr.  Nothing is
// allocated before a launch needs it
struct PeGasRad {
    bool on = false;                            // gcm_set_gas_radiation: registered
    gcm_gas_radiation_par par{};
    double *sc_row = nullptr;                   // device: [Hg]
    int key_kind = -1;
    double key[2] = {0.0, 0.0};
    double *diag = nullptr;                     // device: dt_ground [H][W], olr [H][W]
    int lds_set[2] = {0, 0};                    // the dynamic LDS size the kernel's two forms were last given
};

// Horizontal diffusion (pe25d_hdiff.hip, gcm_set_hdiff): the registration, the device tables of the last (parameters,
// dt) a launch was asked for -- `key`, compared on every step as PeHeldSuarez's -- and the landing fields the launch
// writes, own rows [H][L][W] in the handle's real type, one per state field that was ever selected; they stay until
// gcm_set_hdiff(NULL) or gcm_destroy
struct PeHdiff {
    bool on = false;                            // gcm_set_hdiff: registered
    bool band = false;                          // gcm_set_band_hdiff: a band takes the phase over its own rows
    bool band_done = false;                     // gcm_end_step_diffuse: a band's own rows are diffused for the step gcm_end_step_begin ends
    gcm_hdiff par{};                            // the registration's parameters
    double *tab = nullptr;                      // device: ax bn bs area axv bnv bsv areav, [8][H] (a band: [8][H + 4], rows -2 .. H + 1)
    std::vector<double> key;                    // order, fields, nu, cmax, dt
    int order = 0, fields = 0;                  // what the tables in place were built for
    void *land[GCM_NFIELDS] = {};
};

struct Pe25d {
    gcm_config cfg{};
    int W = 0, H = 0, L = 0, Hg = 0;
    bool wrap = true, f32 = false;
    std::vector<void *> allocs;
    std::vector<double> dsig_host;              // geometry.py dsig, float64 (radiation level tables)
    std::vector<double> sig_host;               // geometry.py sig, float64
    std::vector<double> sigt_host;              // geometry.py sigt, float64 (the height on pressure levels)
    std::vector<double> dxj_host, dxh_host;     // geometry.py dx_j, dx_h over the global height, float64 (horizontal diffusion tables)
    PeBufs<double> d;
    PeBufs<float> f;
    int cur_i = 0;
    bool star_valid = false;
    int nseg = 1;                               // level segments of K4, chosen from the band's size
    int upd_rows = 7;                           // rows per workgroup of K4 (3 or 7)
    int cus = 256;
    int last_stage_set = -1;                    // state set the last half step took its stage state from (gcm_get_intermediate)
    int ghost_ready = -1;                       // state set whose ghost rows' column sums and anchors are queued already (pe25d_prep_ghost_rows)
    int last_unpack_set = -1;                   // state set whose ghost rows the last unpack filled (pe25d_halo_segments)
    bool pit2d = true;                          // pit from the column sums K4 leaves (nseg == 1, row-group K4)
    int nseg_edge = 1;                          // bands: level segments of the EDGE rows' K4 launch (see update_edges)
    bool cs_valid[3] = {false, false, false};   // the state set's column sums belong to its winds
    int pack_set = -1;                          // >= 0: state set gcm_halo_pack reads (step_phase)
    double *stage3 = nullptr;                   // float64 transpose staging, host layout
    double *exner_tab = nullptr;
    double *lev_tab = nullptr;                  // sig [L], dsig [L] in float64, uploaded on first use (pe25d_level_table)
    double *plev_height_tab = nullptr;          // sig [L], dsig [L], sigt [L] in float64, uploaded on first use (pe25d_plev_height.hip)
    FftPlan plan{};
    SuperPlan cplan{};
    double *gt = nullptr;                       // ground temperature [H + 2 ghost rows a side][W], interior row 0 (column physics)
    bool gt_set = false;                        // gcm_set_ground was called
    double *stats_dev = nullptr;                // gcm_stats: block partials, then the area table
    std::vector<double> stats_host, area_host;
    double *rad_tab = nullptr;                  // 5 x [L] level tables of the last radiation call
    double *rad_geo = nullptr;                  // coslat[Hg], sinlat[Hg], lon[W]
    double rad_key[2] = {-1.0, -1.0};           // (t_lw, t_sw) the level tables were built for
    std::vector<double> rad_tab_host, rad_geo_host, rad_latlon;   // host copies (upload sources, change detection)
    std::vector<hipEvent_t> *ev = nullptr;
    size_t *ev_used = nullptr;
    hipStream_t aux = nullptr;                  // second stream of a stage: chain B (K1 + pit, a band's edge rows), see half_t
    hipStream_t aux2 = nullptr;                 // bands: third stream, K1 of the band's OWN rows (no ghost data: off the exchange chain)
    hipEvent_t ev_cs = nullptr;                 // aux2: the own edge rows' column sums of the state just produced are in place
    int edge_cs_set = -1;                       // state set whose own edge rows' column sums were queued on aux2 (nseg_edge > 1)
    bool k1_split = true;                       // GCM_PE_K1_SPLIT=0: K1 of all rows behind the exchange, as in round 3
    bool filter_no_loop = false;                // GCM_PE_FILTER_NO_LOOP (diagnostic): K1 as one workgroup per pair
    bool k4_oddtop = true;                      // GCM_PE_K4_ODDTOP=0: K4's whole columns start on an even level
    bool rad_generic = false;                   // GCM_PE_RAD_GENERIC (diagnostic): the LDS-parked form of the radiation kernel
    // The events a stage's chains hand each other are signalled by the producing kernel's OWN completion
    // (hipExtLaunchKernelGGL's stopEvent) where a kernel is what they follow: a hipEventRecord is a packet of
    // its own behind the kernel and costs the stream 3 us (tools/micro/sync_cost.hip: 8.9 vs 5.9 us per
    // kernel + record; with a stop event 5.95), four of them per stage on the band's long chain.
    bool stop_events = true;                    // GCM_PE_STOP_EVENTS=0: records, as in round 3
    hipEvent_t ev_k4 = nullptr;                 // completion of the last K4 launch on the caller's stream
    bool k4_fork_valid = false;                 // nothing the second stream must follow was queued on the caller's stream since
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // latitude band with registered send buffers: the edge rows of a stage are updated and packed
    // on `aux` while the interior rows run on the caller's stream (pe25d_step_phase)
    void *send_buf[2] = {nullptr, nullptr};
    hipEvent_t ev_a = nullptr, ev_edges = nullptr;
    bool edges_pending = false;
    bool edges_ev_valid = false;                // ev_edges has been recorded at least once (a wait for it means something)
    // gcm_set_band_overlap(1) on a GCM_PE25D band: the interior rows' K4 is held back until chain B has reached the
    // edge rows' K4 (an event recorded right in front of it), so that the edge rows' workgroups are dispatched
    // first: they then take 15-20 us instead of the 60-70 they take when both launches race for the chip, and the
    // pack and the exchange start that much earlier -- at the price of the ~8 us per stage the interior rows wait.
    // Worth it where an exchange takes longer than the ~20 us of slack the edge chain has otherwise; bench.py --gpus N
    // times both on the real ring and keeps the faster.
    bool edges_first = false;
    hipEvent_t ev_pre_edge = nullptr;
    bool pre_edge_pending = false;
    // send / exchange buffers were registered: the format of the ghost-row message, of which the tracers' count and
    // depth are a part, is fixed
    bool halo_fixed = false;
    PeTracers tr;
    PeHeldSuarez hs;
    PeSampler clim;                             // the four sampled diagnostics, in the order a step samples (PeSample)
    PePlev plev;
    PeSpectra spec;
    PePlev pmaps;
    PeMoist moist;
    PeConvect convect;
    PeBettsMiller betts_miller;
    PeBoundary boundary;
    PeSlab slab;
    PeGasRad gas;
    PeHdiff hdiff;
};

template <typename T> inline PeBufs<T> &bufs(Pe25d *m);
template <> inline PeBufs<double> &bufs<double>(Pe25d *m) { return m->d; }
template <> inline PeBufs<float> &bufs<float>(Pe25d *m) { return m->f; }

inline size_t elem_size(const Pe25d *m) { return m->f32 ? sizeof(float) : sizeof(double); }
// field f of state set `set` in the handle's real type, at interior row 0
inline void *state_field(const Pe25d *m, int set, int f) { return m->f32 ? (void *)m->f.st[set][f] : (void *)m->d.st[set][f]; }

// a band's tracer fields: the declared ghost rows a side (gcm_set_band_tracer_rows).  One by default: pe_tracer_kernel
// reads rows j - 1 .. j + 1 only, and so does the donor-cell scheme; the van Leer scheme reads j -+ 2 and is refused
// on a band that declared fewer than two.  A single domain: none.  The storage, the message (tracer_halo_bytes,
// tracer_halo_segments) and set / get all take the depth from here
inline int tr_ghost(const Pe25d *m) { return m->wrap ? 0 : m->tr.rows; }
// the deepest a band's tracers may be declared: what the van Leer scheme reads.  It may not exceed the state's ghost
// depth: the edge launch of update_edges covers kGhost own rows a side, which are the rows a neighbour takes and the
// only rows that may read tracer ghost rows
constexpr int kTrGhostMax = 2;
static_assert(kTrGhostMax <= kGhost, "the tracers' edge launch covers kGhost rows a side");
inline long tr_stride(const Pe25d *m) { return (long)(m->H + 2 * tr_ghost(m)) * m->L * m->W; }
// tracer f of set 0 (current) or 1 (star), at interior row 0
inline char *tr_field(const Pe25d *m, int set, int f) {
    return (char *)m->tr.buf + elem_size(m) * ((size_t)(set * m->tr.n + f) * tr_stride(m) + (size_t)tr_ghost(m) * m->L * m->W);
}

template <typename T>
inline bool dev_upload(Pe25d *m, T **dst, const T *src, size_t count) {
    void *d = nullptr;
    if (hipMalloc(&d, count * sizeof(T)) != hipSuccess) return false;
    m->allocs.push_back(d);
    if (src && hipMemcpy(d, src, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return false;
    if (!src && hipMemset(d, 0, count * sizeof(T)) != hipSuccess) return false;
    *dst = (T *)d;
    return true;
}

// a HIP status as an entry point's return code, the message prefixed with the entry point's name
inline int hip_rc(hipError_t e, const char *fn, std::string *err) {
    if (e == hipSuccess) return GCM_OK;
    *err = std::string("hip: ") + fn + ": " + hipGetErrorString(e);
    return GCM_ERR_HIP;
}

inline size_t rows_alloc(const Pe25d *m) { return (size_t)m->H + 2 * kGhost; }

template <typename T>
inline size_t upd_lds_bytes(int R, int L) { return sizeof(T) * ((size_t)3 * (11 * R + 11) * 64 + 2 + 4 * (size_t)L); }
// looping filter kernels: the complex row + iph(sp) of the row + the row's multiplier
template <typename T>
inline size_t filter_loop_lds_bytes(const Pe25d *m) {
    return (size_t)m->W * sizeof(typename Vec2<T>::type) + ((size_t)m->W + m->W / 2 + 1) * sizeof(T);
}
template <typename T>
inline size_t filter_lds_bytes(const Pe25d *m) {
    return (size_t)(m->cplan.ok ? 1 : 2) * m->W * sizeof(typename Vec2<T>::type);
}
// pe_pit2d_kernel: the composite path keeps the filtered row after its one-row workspace, the generic path in the
// free half of its two (pe_pit2d_row)
template <typename T>
inline size_t pit2d_lds_bytes(const Pe25d *m) {
    return filter_lds_bytes<T>(m) + (m->cplan.ok ? sizeof(T) * (size_t)m->W : 0);
}

template <typename T>
inline PeArgsT<T> make_args(Pe25d *m, int stage_set, int out_set, double dt) {
    PeBufs<T> &Bf = bufs<T>(m);
    PeArgsT<T> a{};
    T *const *B = Bf.st[m->cur_i];
    T *const *S = Bf.st[stage_set];
    T *const *O = Bf.st[out_set];
    a.p = B[GCM_P]; a.u = B[GCM_U]; a.v = B[GCM_V]; a.t = B[GCM_T]; a.q = B[GCM_Q];
    a.sp = S[GCM_P]; a.su = S[GCM_U]; a.sv = S[GCM_V]; a.st = S[GCM_T]; a.sq = S[GCM_Q];
    a.op = O[GCM_P]; a.ou = O[GCM_U]; a.ov = O[GCM_V]; a.ot = O[GCM_T]; a.oq = O[GCM_Q];
    a.spu = Bf.spu; a.phi = Bf.phi; a.pgfu = Bf.pgfu;
    a.pit = Bf.pit; a.pn = Bf.pn;
    a.scs_u = Bf.cs[stage_set][0]; a.scs_v = Bf.cs[stage_set][1];
    a.ocs_u = a.ocs_v = nullptr;
    a.part = Bf.part;
    a.part_stride = (long)rows_alloc(m) * m->W;
    a.nseg = m->nseg;
    a.spu_j0 = a.pit_j0 = -(1 << 30);            // K1: every row of the launch
    a.spu_j1 = a.pit_j1 = 1 << 30;
    a.inv_dxj = Bf.inv_dxj; a.inv_dxh = Bf.inv_dxh;
    a.sig = Bf.sig; a.dsig = Bf.dsig; a.inv_dsig = Bf.inv_dsig; a.sigb = Bf.sigb; a.sigt = Bf.sigt;
    a.heightmap = Bf.heightmap; a.cor_u = Bf.cor_u; a.cor_v = Bf.cor_v; a.smul = Bf.smul; a.tw = Bf.tw;
    a.exner_tab = m->exner_tab;
    a.plan = m->plan;
    a.cplan = m->cplan;
    a.W = m->W; a.H = m->H; a.L = m->L; a.Hg = m->Hg; a.row0 = m->cfg.row0;
    a.wrap = m->wrap ? 1 : 0;
    a.filter = m->cfg.filter;
    a.dt = (T)dt;
    a.inv_dy = (T)(1.0 / m->cfg.dy);
    a.ptop = (T)m->cfg.ptop;
    return a;
}

// The dynamic LDS size of every kernel a unit launches with more than the default, set where the kernel is
// instantiated: the filter, pit2d and K4 kernels and pe_geopot_kernel<T, 0> (pe25d_kernels.hip), pe_radiation_kernel<T, 0>
// (pe25d_physics.hip).  pe25d_create calls both; false: hipFuncSetAttribute failed
bool stage_lds_attributes(const Pe25d *m);
bool radiation_lds_attribute(const Pe25d *m);

// What the moist physics and the convective adjustment share (pe25d_state.hip).  pe25d_level_table: sig [L], then dsig
// [L], in float64 on the device, uploaded by the first call; null with *err = "hip: <who> table upload failed".
// pe25d_phase_wrote: the handle's bookkeeping behind a launch that changes state set `set` in place, see there
const double *pe25d_level_table(Pe25d *m, const char *who, std::string *err);
void pe25d_phase_wrote(Pe25d *m, int set, bool keep_ghosts, bool wrote_uv);

// Host layout [levels][H][W], float64, <-> a device field [j][levels][i] of the handle's own rows in its real type: the
// copy through the staging buffer and the transpose, queued on `s`; the caller synchronises (pe25d_state.hip)
hipError_t field_to_device(Pe25d *m, void *dev_field, const double *host, int levels, hipStream_t s);
hipError_t field_to_host(Pe25d *m, double *host, const void *dev_field, int levels, hipStream_t s);

// One segment of a ghost-row message, appended to *c: the `rows` edge rows of one side (0 = north) of a field of H own
// rows go to the message at *msg (pack), or the message's rows to the field's ghost rows (unpack); *msg moves on.  base =
// the field's own row 0, words = 8-byte words a row (SegCopy moves those: rows x even W floats are a whole number of them)
inline void halo_segment(SegCopy *c, bool pack, int side, void *base, int H, int rows, size_t words, double **msg) {
    double *const b = (double *)base;
    double *const edge = side == 0 ? b : b + (size_t)(H - rows) * words;
    double *const ghost = side == 0 ? b - (size_t)rows * words : b + (size_t)H * words;
    c->src[c->nseg] = pack ? edge : *msg;
    c->dst[c->nseg] = pack ? *msg : ghost;
    c->n[c->nseg++] = (long)(rows * words);
    *msg += rows * words;
}

// ---------------------------------------------------------------- the tracers' host side (pe25d_tracers.hip)
// the passive tracers of one stage over rows [r0, r1) and [rb0, rb1) on `st`; `a`: the stage's arguments
template <typename T>
void launch_tracers(Pe25d *m, const PeArgsT<T> &a, int stage_set, int out_set, hipStream_t st, int r0, int r1, int rb0 = 0, int rb1 = 0);
// hazard 1 (with pe25d_join_tracers / pe25d_follow_tracers): the last stage's tracer launch on another stream may still
// run (Stage::tr_prev); `st` must follow it before anything queued there overwrites what it reads or reads what it wrote
bool last_tracers_in_flight(const Pe25d *m);
void follow_last_tracers(Pe25d *m, hipStream_t st);
// the tracer launch just queued on `st` is the stage's whole (mode 0) or interior (mode 1) launch: the next stage
// follows it (follow_last_tracers); caller_joins: so does the caller's stream in pe25d_join_tracers
void stage_tracers_launched(Pe25d *m, hipStream_t st, bool caller_joins);
// a band's tracers in the ghost-row message: their bytes a side, and their segments of state set `set`
size_t tracer_halo_bytes(const Pe25d *m);
void tracer_halo_segments(Pe25d *m, bool pack, int side, int set, double **msg, SegCopy *c);
void tracers_destroy(Pe25d *m);                  // pe25d_destroy: the tracers' storage, forcing, mixing and events
// hazard 4 (pe25d_convect_tracers.hip): the tracers' convective mixing writes the current tracers on the caller's stream,
// ahead of the adjustment's launch (pe25d_convect_rows calls it).  It joins the last stage's tracer launches first
// (pe25d_join_tracers); the next stage's tracer launch on the second stream follows it because the launch invalidates the
// fork at the last K4 (pe25d_fork_invalidate: chain B then waits for the caller's stream's position) -- the invalidation
// was chosen, not an event of its own: nothing is recorded, and a step without opt-ins queues what it queued
int pe25d_convect_tracers_rows(Pe25d *m, int set, int j0, int j1, hipStream_t s, std::string *err);
void tracers_convect_forget(Pe25d *m);           // the tracers' storage went: so do the opt-ins

}  // namespace gcm

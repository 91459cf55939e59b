/* gcmcore.h -- C ABI of libgcmcore.so, the MI355X-native Matsuno C-grid
 * dynamical core for gcmiipy.
 *
 * The reference (marthinwurer/gcmiipy) is pure Python/NumPy and has no FFI of
 * its own; the entry points below are what a ctypes binding for its time-step
 * functions needs (INTEGRATION.md shows that binding).  Each one names the
 * reference interface it stands behind.  Plain pointers and sizes only; no
 * torch / numpy types.  Every function returns 0 on success or a negative
 * gcm_status; nothing throws across the ABI; the message of the last failure
 * is available from gcm_last_error().
 *
 * Threading: a handle is driven by one host thread at a time.  Calls that
 * launch work (gcm_step, gcm_half_step, gcm_halo_*) are asynchronous on the
 * handle's stream; gcm_get_state / gcm_diag / gcm_sync synchronise.
 *
 * Memory: all arrays are float64, C-contiguous, reference layout:
 *   2-D fields [j][i]   (H rows x W columns, i fastest)
 *   3-D fields [k][j][i] (L levels, k = 0 is the bottom layer)
 * Host buffers stay caller-owned and are only touched inside set/get calls.
 */
#ifndef GCMCORE_H
#define GCMCORE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCM_ABI_VERSION 1

typedef struct gcm_handle gcm_handle;

typedef enum {
    GCM_OK = 0,
    GCM_ERR_ARG = -1,      /* bad argument / shape (mirrors the reference's shape asserts) */
    GCM_ERR_HIP = -2,      /* a HIP runtime call failed                                     */
    GCM_ERR_NODEVICE = -3, /* no gfx950 device visible: there is NO CPU fallback            */
    GCM_ERR_STATE = -4,    /* call sequence error (e.g. half_step corrector before predictor) */
    GCM_ERR_UNSUPPORTED = -5
} gcm_status;

/* Which reference time-step the handle integrates. */
typedef enum {
    GCM_SW2D = 1,      /* matsuno_c_grid.matsumo_scheme(u,v,p,dx,dt)        matsuno_c_grid.py:125-142 */
    GCM_SW2D_TEMP = 2, /* matsumo_temp.matsumo_scheme(u,v,p,t,dx,dt)        matsumo_temp.py:66-99
                          (+ optional tracer q, two_d.py:198-207 / flux_limiter.py:10-32)            */
    GCM_PE2D = 3,      /* no_limits_2d.matsuno_timestep(p,u,v,t,q,dt,dx)    no_limits_2d.py:129-131   */
    GCM_PE25D = 4      /* dynamics.matsuno_timestep(p,u,v,t,q,dt,geom)      dynamics.py:230-237       */
} gcm_model;

typedef enum { GCM_P = 0, GCM_U = 1, GCM_V = 2, GCM_T = 3, GCM_Q = 4, GCM_NFIELDS = 5 } gcm_field;

/* Tracer scheme carried by GCM_SW2D_TEMP alongside the dynamics (advected by
 * the time-n winds, V = (v, u) in two_d.py's axis convention). */
typedef enum {
    GCM_TRACER_NONE = 0,
    GCM_TRACER_UPWIND = 1,  /* two_d.finite_volume_advection            two_d.py:198-207          */
    GCM_TRACER_VANLEER = 2  /* the same split step with van_leer(calc_r) limiting of the centred
                               flux (flux_limiter.py:10-20, two_d.py:135-149); composition by this
                               build, see DESIGN.md                                               */
} gcm_tracer;

typedef enum { GCM_F64 = 0, GCM_F32 = 1 } gcm_dtype;

/* Kernel variant (same arithmetic, different data movement). */
typedef enum {
    GCM_VARIANT_AUTO = 0,
    GCM_VARIANT_STAGED = 1, /* one launch per Matsuno stage, predicted state materialised in HBM */
    GCM_VARIANT_FUSED = 2   /* predictor + corrector in one launch, predicted state in registers */
} gcm_variant;

typedef struct {
    int32_t abi_version;   /* GCM_ABI_VERSION */
    int32_t model;         /* gcm_model */
    int32_t width;         /* W: cells along i (longitude), contiguous                          */
    int32_t height;        /* H: rows along j owned by THIS handle (a latitude band if nranks>1) */
    int32_t layers;        /* L: sigma levels (GCM_PE25D), else 1                                */
    int32_t tracer;        /* gcm_tracer (GCM_SW2D_TEMP only)                                    */
    int32_t variant;       /* gcm_variant                                                        */
    int32_t filter;        /* GCM_PE25D: 1 = apply low_pass.arakawa_1977 (low_pass.py:41-78)     */
    /* Latitude-band decomposition.  nranks == 1: the handle owns the whole grid
     * and np.roll's pole-to-pole periodicity along j is done by index arithmetic.  nranks > 1:
     * rows [row0, row0+height) of a global_height-row grid; the ghost rows on either side
     * are filled by the caller between steps through gcm_halo_* (RCCL ring incl. the wrap).    */
    int32_t nranks;
    int32_t rank;
    int32_t global_height;
    int32_t row0;
    int32_t device;        /* HIP device ordinal; -1 = current                                   */
    int32_t dtype;         /* gcm_dtype: GCM_F64 (default) or GCM_F32: arithmetic and storage in fp32.
                              Honoured by GCM_PE25D, GCM_SW2D and GCM_SW2D_TEMP (any tracer, variant,
                              ensemble or band); GCM_PE2D and the stand-alone operators stay fp64.  The
                              host API stays float64: uploads round to nearest-even, downloads widen
                              exactly.  Other values: GCM_ERR_ARG from GCM_SW2D, GCM_SW2D_TEMP and
                              GCM_PE25D (GCM_PE2D ignores the field).  fp32 2-D latitude bands of odd
                              width: GCM_ERR_UNSUPPORTED                                           */
    int32_t halo_steps;    /* 2-D bands: Matsuno steps per ghost-row exchange (ghost depth = 2 *
                              halo_steps rows per side, deep-halo communication avoiding); 0/1 = 1 */
    int32_t members;       /* ensemble members M of GCM_SW2D / GCM_SW2D_TEMP (single band): M independent states
                              on one grid with one dx, model, tracer and dt, all advanced by each launch; 0/1 = 1.
                              Negative: GCM_ERR_ARG; > 1 with GCM_PE2D, GCM_PE25D or nranks > 1: GCM_ERR_UNSUPPORTED */
    double dx;             /* scalar grid spacing in metres (2-D models: both axes)              */
    double dy;             /* GCM_PE25D: geom.dy                            geometry.py:138      */
    double ptop;           /* GCM_PE25D: geom.ptop in Pa                    geometry.py:147      */
    /* GCM_PE25D host tables, copied at create (geometry.py:79-85,136-137,149): */
    const double *dx_j;    /* [global_height]  zonal spacing at cell-centre latitudes            */
    const double *dx_h;    /* [global_height]  zonal spacing at v latitudes                      */
    const double *sig;     /* [L] */
    const double *dsig;    /* [L] */
    const double *sigb;    /* [L] */
    const double *sigt;    /* [L] */
    const double *heightmap; /* [global_height][W] (all rows), or NULL for flat topography       */
    /* Coriolis terms of advec_m_pu (dynamics.py:82-92; switched off by `if False` in the
     * reference): cor_u[j] = 2 sin(lat_j) w, cor_v[j] = 2 sin(jph(lat)_j) w, w = 2 pi / day.
     * Both NULL = the reference's literal 0.                                                   */
    const double *cor_u;   /* [global_height] */
    const double *cor_v;   /* [global_height] */
    void *stream;          /* hipStream_t to launch on; NULL = the null stream                   */
} gcm_config;

/* Library / device probes (no handle needed). */
int gcm_abi_version(void);
int gcm_device_count(void);                 /* gfx950 devices visible; 0 on a CPU-only box */
const char *gcm_build_info(void);           /* compiler, offload arch, build flags          */
/* The 256-double table the kernels use for (p/P0)**kappa (temperature.py:7-19): lets a host
 * test check the device algorithm's accuracy without a GPU.  Returns 0. */
int gcm_exner_table(double *out256);
/* The composite-radix plan of the polar filter's in-LDS transform (low_pass.py:41-78 does numpy.fft.rfft /
 * irfft; csrc/fft_lds.h) for rows of n columns, so that a host test can replay the passes' index arithmetic
 * without a GPU.  out[0] = 1 if the composite path serves n (0: generic mixed-radix path), out[1] = passes,
 * out[2] = threads per workgroup, then four words per pass: r1, r2 (the pass has radix r1 * r2),
 * magic = ceil(2^32 / Ns) of the forward pass, imagic = the same for the inverse transform, whose passes take
 * the radices in reversed order.  cap = words available in out (>= 3 + 4 * 8).  Returns 0. */
int gcm_filter_plan(int n, unsigned *out, int cap);

/* Lifetime.  Device buffers are library-owned inside the handle. */
int gcm_create(const gcm_config *cfg, gcm_handle **out);
int gcm_destroy(gcm_handle *h);
const char *gcm_last_error(const gcm_handle *h); /* h may be NULL: last create() failure */

/* State transfer (host <-> device).  NULL pointers are skipped.  Fields a model
 * does not have must be NULL.  2-D models: all five are [H][W] ([M][H][W] on an
 * ensemble handle, members M > 1, here and in gcm_get_star / gcm_set_star); GCM_PE25D: p is
 * [H][W], the rest [L][H][W].  Reference tuple orders: (u,v,p[,t]) for the
 * shallow-water schemes, (p,u,v,t,q) for the primitive-equation ones.          */
int gcm_set_state(gcm_handle *h, const double *p, const double *u, const double *v,
                  const double *t, const double *q);
int gcm_get_state(gcm_handle *h, double *p, double *u, double *v, double *t, double *q);

/* Ensembles (config.members > 1): gcm_members gives M (1 for any other handle).  gcm_set_member /
 * gcm_get_member move member m's [H][W] fields alone (0 <= m < M, else GCM_ERR_ARG), so a caller can
 * perturb or read one member without copying all M.  gcm_diag_members fills out[m] with gcm_diag's
 * value of every member (n >= M), by one launch and one synchronisation; gcm_diag on an ensemble
 * handle reduces over all members.  gcm_snapshot / gcm_restore cover all members.                  */
int gcm_members(const gcm_handle *h);
int gcm_set_member(gcm_handle *h, int m, const double *p, const double *u, const double *v,
                   const double *t, const double *q);
int gcm_get_member(gcm_handle *h, int m, double *p, double *u, double *v, double *t, double *q);

/* One or more full Matsuno steps (predictor + corrector), state stays resident.
 * Stands behind matsumo_scheme / matsuno_timestep (files cited at gcm_model). */
int gcm_step(gcm_handle *h, int nsteps, double dt);

/* What gcm_step(h, nsteps, .) of a 2-D handle would launch, without launching anything: a read-only query for tests
 * and tools, taken from the expressions gcm_step and the kernel launchers use themselves (GCM_SW2D_TWO_STEP, read per
 * call, and the per-launch timing of gcm_time_steps included).  out (nout >= GCM_SW2D_PLAN_WORDS words):
 *   [0] the variant, GCM_VARIANT_FUSED or GCM_VARIANT_STAGED; [1] .. [4] are 0 for the staged variant
 *   [1] rows per band (output rows per wave)      [2] columns per lane (2: fp32 with an even width)
 *   [3] strip width in columns of the single-step kernel (60 x columns per lane)
 *   [4] strip width in columns of the two-step kernel (56)
 *   [5] two-step launches (each advances two steps)  [6] steps taken one at a time: nsteps - 2 x [5]
 *   [7] 1: the single-step kernel is the preloading form (plain GCM_SW2D, bands of up to 4 rows), 0: the rolling form
 *   [8] 1: the rolling form's STREAM instantiation (one launch reads more than 256 MB)
 * A latitude band: the rows of its next step.  A GCM_PE25D handle, a null pointer, nsteps < 0 or nout too small:
 * GCM_ERR_ARG.                                                                                                 */
#define GCM_SW2D_PLAN_WORDS 9
int gcm_sw2d_plan(gcm_handle *h, int nsteps, int *out, int nout);

/* Rows of requests a wave of the single-step fused kernel keeps in flight on the handle's next step: 1, or 3 -- the
 * deep march at two waves per SIMD -- where the launch is the STREAM instantiation of a float64 GCM_SW2D_TEMP handle.
 * GCM_SW2D_DEPTH = 1 | 3, read by gcm_create, pins it for float64 GCM_SW2D_TEMP handles of any size; every other
 * handle ignores the switch.  0: the staged variant.  A GCM_PE25D handle or a null pointer: GCM_ERR_ARG.         */
int gcm_sw2d_fused_depth(gcm_handle *h);

/* The wave pair of float64 GCM_SW2D_TEMP (fused, one member, a periodic single domain): two steps per launch, which
 * gcm_sw2d_plan reports through its words [5] and [6].  out (nout >= GCM_SW2D_PAIR_WORDS words):
 *   [0] 1: a gcm_step call of two or more steps goes through it (GCM_SW2D_PAIR = 0 | 1, read by gcm_create, pins it
 *       at any size; unset: the library's default for grids whose launches stream), 0: it does not
 *   [1] its own band length in rows (one resident round of workgroups, or GCM_SW2D_PAIR_ROWS, read by gcm_create);
 *       0: a handle the pair never serves
 * A GCM_PE25D handle, a null pointer or nout too small: GCM_ERR_ARG.                                            */
#define GCM_SW2D_PAIR_WORDS 2
int gcm_sw2d_pair_info(gcm_handle *h, int *out, int nout);

/* The launch geometry of the GCM_PE25D phases whose grid depends on the rows of the launch, the row length and the
 * chip's compute units, without launching anything: a read-only query for tests and tools, taken from the helpers the
 * launchers use themselves.  gcm_pe25d_phase_geometry needs no handle and no device: a launch over `rows` rows of W
 * columns and L levels on a chip of `cus` compute units, elem_bytes 8 (fp64) or 4 (fp32).  accumulate: GCM_PHASE_MOIST
 * only -- 1: the launch adds to the registered sums (own rows) and marches whole columns; 0: it does not (a band's ghost
 * rows, an unregistered gcm_moist_step) and splits the levels.  out (nout >= GCM_PHASE_PLAN_WORDS words, unused ones 0):
 *   GCM_PHASE_HELD_SUAREZ, GCM_PHASE_MOIST: [0] grid x (256-column blocks)  [1] grid y (rows)  [2] grid z = level
 *     segments nseg; segment s marches levels [s L / nseg, (s + 1) L / nseg), four at a time
 *     [3] the fewest, [4] the most levels of a segment
 *   GCM_PHASE_CLIMATE (rows = the handle's own rows H): [0] grid x = rows  [1] level segments nseg (grid y)
 *     [2] the fewest, [3] the most levels a workgroup walks  [4] iterations of a level's loop over 3 x 256 columns
 *   GCM_PHASE_TRACER_FORCING (one run of rows x L x W elements that starts on 16 bytes): [0] workgroups per forced
 *     tracer  [1] passes of the whole 16-byte vectors over that grid
 * gcm_pe25d_phase_plan is the same for a GCM_PE25D handle's own W, L, element size and compute units; rows < 0: the
 * handle's own rows H (the explicit phase calls of a band launch H + 4: its ghost rows too).  An unknown phase, a size
 * < 1, a null pointer, nout too small: GCM_ERR_ARG; a handle of another model: GCM_ERR_UNSUPPORTED.                     */
typedef enum { GCM_PHASE_HELD_SUAREZ = 0, GCM_PHASE_MOIST = 1, GCM_PHASE_CLIMATE = 2, GCM_PHASE_TRACER_FORCING = 3 } gcm_pe25d_phase;
#define GCM_PHASE_PLAN_WORDS 5
int gcm_pe25d_phase_geometry(int phase, int W, int rows, int L, int cus, int elem_bytes, int accumulate, int *out, int nout);
int gcm_pe25d_phase_plan(gcm_handle *h, int phase, int rows, int accumulate, int *out, int nout);

/* The launch geometry of the GCM_PE25D dynamics stage where it depends on the rows, the level count, the row's filter
 * plan and the chip's compute units, without launching anything: a read-only query for tests and tools, taken from the
 * helpers the launchers use themselves.  K1 is the looping filter kernel (spu = filter(su iph(sp)), with pit in one more
 * workgroup a row), K4 the row-group update kernel.  gcm_pe25d_stage_geometry needs no handle and no device: a
 * whole-domain stage over `rows` rows of W columns and L levels on a chip of `cus` compute units at the default
 * switches, elem_bytes 8 (fp64) or 4 (fp32); plan / nplan: the words gcm_filter_plan writes for W, or NULL for the
 * library's own plan of W.  out (nout >= GCM_STAGE_PLAN_WORDS words, unused ones 0), by GCM_STAGE_*:
 *   K1_LOOP 1: the looping form (0: one workgroup per level pair; the instantiation words are then 0)
 *   K1_MAXR, K1_MASK (0, 1440, 2880 or 4096: the plan the instantiation is compiled for), K1_NIN, K1_NW: the
 *     instantiation pe_spu_filter_loop_kernel<T, MAXR, MASK, NIN, NW>;  K1_PASSES: passes of the row's composite plan
 *   K1_WGS_PER_ROW workgroups a row that filter, each looping over K1_PAIRS_PER_WG level pairs, the last one over
 *     K1_PAIRS_LAST_WG (an odd L: its last pair is a single level);  K1_PIT_RIDES 1: pit and p_n in the same launch
 *   K4_ROWS rows per workgroup (3 or 7), K4_GROUPS row groups, the last of K4_ROWS_LAST_GROUP rows; K4_COL_TILES tiles
 *     of 62 columns, the last of K4_COLS_LAST_TILE; K4_NSEG level segments; K4_ODDTOP 1: the march starts on an odd
 *     level; K4_GRID workgroups launched (padded to the 8 XCDs)
 * gcm_pe25d_stage_plan is the same for what a GCM_PE25D handle launches for a stage over all its rows (mode 0), with the
 * handle's GCM_PE_* switches.  A band (nranks > 1) that splits its stage into edge rows and interior rows also reports
 *   BAND 1;  K1_SPLIT 1: inside gcm_band_run K1 of the own rows is a launch of its own, K1_OWN_WGS_PER_ROW workgroups
 *     a row x K1_OWN_PAIRS_PER_WG pairs, the last K1_OWN_PAIRS_LAST_WG
 *   K4_EDGE_GROUPS, K4_EDGE_ROWS_LAST_GROUP, K4_EDGE_ODDTOP, K4_EDGE_GRID: K4 of the two edge rows of either side, one
 *     launch over two row ranges in NSEG_EDGE level segments;  K4_INT_*: the same words for K4 of the interior rows
 * A size < 1, a null `out`, plan words that are no plan, nout too small: GCM_ERR_ARG; a handle of another model:
 * GCM_ERR_UNSUPPORTED.                                                                                                 */
enum {
    GCM_STAGE_K1_LOOP = 0, GCM_STAGE_K1_MAXR = 1, GCM_STAGE_K1_MASK = 2, GCM_STAGE_K1_NIN = 3, GCM_STAGE_K1_NW = 4,
    GCM_STAGE_K1_PASSES = 5, GCM_STAGE_K1_WGS_PER_ROW = 6, GCM_STAGE_K1_PAIRS_PER_WG = 7, GCM_STAGE_K1_PAIRS_LAST_WG = 8,
    GCM_STAGE_K1_PIT_RIDES = 9,
    GCM_STAGE_K4_ROWS = 10, GCM_STAGE_K4_GROUPS = 11, GCM_STAGE_K4_ROWS_LAST_GROUP = 12, GCM_STAGE_K4_COL_TILES = 13,
    GCM_STAGE_K4_COLS_LAST_TILE = 14, GCM_STAGE_K4_NSEG = 15, GCM_STAGE_K4_ODDTOP = 16, GCM_STAGE_K4_GRID = 17,
    GCM_STAGE_BAND = 18, GCM_STAGE_K1_SPLIT = 19, GCM_STAGE_K1_OWN_WGS_PER_ROW = 20, GCM_STAGE_K1_OWN_PAIRS_PER_WG = 21,
    GCM_STAGE_K1_OWN_PAIRS_LAST_WG = 22,
    GCM_STAGE_K4_EDGE_GROUPS = 23, GCM_STAGE_K4_EDGE_ROWS_LAST_GROUP = 24, GCM_STAGE_K4_EDGE_ODDTOP = 25,
    GCM_STAGE_K4_EDGE_GRID = 26, GCM_STAGE_NSEG_EDGE = 27,
    GCM_STAGE_K4_INT_GROUPS = 28, GCM_STAGE_K4_INT_ROWS_LAST_GROUP = 29, GCM_STAGE_K4_INT_ODDTOP = 30,
    GCM_STAGE_K4_INT_GRID = 31
};
#define GCM_STAGE_PLAN_WORDS 32
int gcm_pe25d_stage_geometry(int W, int rows, int L, int cus, int elem_bytes, const unsigned *plan, int nplan, int *out, int nout);
int gcm_pe25d_stage_plan(gcm_handle *h, int *out, int nout);

/* One Euler stage, for per-stage parity tests and for the reference's
 * boundary_conditions hook (dynamics.py:232-236): stage == 0 computes the
 * predictor from the current state into the handle's "star" buffers; stage == 1
 * computes the corrector from (current, star) and makes it the current state.
 * gcm_get_star / gcm_set_star expose the predicted state in between.
 * Stands behind half_timestep (dynamics.py:183-227, no_limits_2d.py:104-126). */
int gcm_half_step(gcm_handle *h, int stage, double dt);
int gcm_get_star(gcm_handle *h, double *p, double *u, double *v, double *t, double *q);
int gcm_set_star(gcm_handle *h, const double *p, const double *u, const double *v,
                 const double *t, const double *q);

/* Passive tracers of GCM_PE25D: n fields c[n][L][H][W] that every Matsuno stage of gcm_step /
 * gcm_half_step / gcm_time_steps (a latitude band: gcm_band_run, gcm_step_phase, gcm_step_interior /
 * gcm_step_boundary) advances with exactly the update the reference applies to q
 * (dynamics.py:219, advec_t :174-181, advec_sig :49-52) on the stage's own mass fluxes:
 *     c_n = (c p - (advec_t(spu, spv, sc) + advec_sig(sd, sc)) dt) / p_n,   sc = the stage value,
 * so a tracer equal to q stays equal to q (bit for bit in fp64).  That update takes centred face values: no flux
 * limiting, no positivity (the reference applies none to q); gcm_set_tracer_scheme below selects donor-cell or
 * van Leer limited face values for the tracers.  The handle stores them in its own real type; the host API is float64.
 * gcm_set_tracers: 0 <= n <= GCM_MAX_TRACERS (n = 0 frees them), also resets the star set to c;
 * gcm_get_tracers: which = 0 the current tracers, 1 those of the last predictor (GCM_ERR_STATE before
 * one); gcm_tracer_count: n.  Other models: GCM_ERR_UNSUPPORTED.  On a latitude band (nranks > 1) c holds
 * the band's own rows (H = height) and n must equal the count declared by gcm_set_band_tracers; without a
 * declaration (or with 0) gcm_set_tracers returns GCM_ERR_UNSUPPORTED, any other n GCM_ERR_ARG.  On a band
 * gcm_set_tracers (like gcm_set_state) makes the next gcm_band_run exchange the ghost rows first.
 * The tracer kernel runs on the handle's second (a band's: second and third) stream; these calls,
 * gcm_step, gcm_half_step, gcm_band_run and gcm_sync include it.  Without tracers the step is the same
 * work as before.                                                                                      */
#define GCM_MAX_TRACERS 16
int gcm_set_tracers(gcm_handle *h, int n, const double *c);
int gcm_get_tracers(gcm_handle *h, int which, double *c);
int gcm_tracer_count(const gcm_handle *h);
/* The transport scheme of the passive tracers of a GCM_PE25D handle (q keeps the reference's update in every case).
 * The update keeps its flux form, its mass fluxes (spu, spv, sigma-dot) and its divisor p_n; the scheme is the value
 * of the stage tracer sc that a mass flux F carries through the face between cells A and B (F > 0: from A to B), in
 * all three directions from the one stage field (no dimension splitting):
 *   GCM_TRACER_NONE (default)  (sc[A] + sc[B]) / 2, the update above;
 *   GCM_TRACER_UPWIND          sc[U], U = A if F > 0 (strict) else B                    flux_limiter.py:23-27
 *   GCM_TRACER_VANLEER         sc[U] + 1/2 phi(r) (sc[D] - sc[U]), phi(r) = (r + |r|) / (1 + |r|),
 *                              r = (sc[U] - sc[UU]) / (sc[D] - sc[U]), 0 where that denominator is 0
 *                              (D: the other cell of the face, UU: the cell behind U)    flux_limiter.py:10-20
 * Differences are plain differences of neighbouring cells.  i is periodic, rows wrap as in the centred update; the
 * column does not wrap: a level face whose UU lies outside the column is donor-cell.
 * gcm_set_tracer_scheme: at any time between steps, with or without tracers set; it includes the tracer stream
 * first, as gcm_set_tracers does, and leaves no predicted tracers (gcm_get_tracers(which = 1): GCM_ERR_STATE until the
 * next predictor).  Errors: an unknown scheme GCM_ERR_ARG; a model other than GCM_PE25D GCM_ERR_UNSUPPORTED;
 * GCM_TRACER_VANLEER on a latitude band (nranks > 1) that has not declared two tracer ghost rows per side
 * (gcm_set_band_tracer_rows(h, 2), below) GCM_ERR_UNSUPPORTED: it reads rows j -+ 2, and a band's tracers carry one
 * ghost row per side unless told otherwise (GCM_TRACER_UPWIND reads j -+ 1 and runs on any band; every band of a run
 * must be given the same scheme).  A refused call leaves the scheme in force as it was.
 * gcm_tracer_scheme: the scheme in force (other models: GCM_TRACER_NONE).                                */
int gcm_set_tracer_scheme(gcm_handle *h, int scheme);
int gcm_tracer_scheme(const gcm_handle *h);
/* GCM_PE25D latitude bands (nranks > 1): the number of passive tracers the band carries, 0..GCM_MAX_TRACERS.
 * Fixes the ghost-row message (gcm_halo_bytes) and so must come before gcm_set_halo_buffers / gcm_set_exchange.
 * The band's tracers start as zeros (gcm_set_tracers with the same n sets them).  Errors: n out of range
 * GCM_ERR_ARG; any handle but a GCM_PE25D band (single domains need no declaration) GCM_ERR_UNSUPPORTED;
 * a call after send or exchange buffers were registered GCM_ERR_STATE.                                 */
int gcm_set_band_tracers(gcm_handle *h, int n);
/* GCM_PE25D latitude bands: the ghost rows per side that the band's tracers carry, rows = 1 (default: the message
 * format of gcm_set_band_tracers, byte for byte) or 2 (what GCM_TRACER_VANLEER reads; gcm_set_tracer_scheme accepts
 * it on a band only at this depth).  The depth is a declaration of its own, not a consequence of the scheme: the
 * scheme may change between any two steps, the message size may not change once buffers are registered.  Same life
 * cycle as gcm_set_band_tracers: before gcm_set_halo_buffers / gcm_set_exchange, before or after
 * gcm_set_band_tracers, and either may be repeated until then.  A change of depth includes the tracer stream first
 * and allocates the band's tracers anew, as zeros.  With rows = 2 the centred and the donor-cell scheme compute what
 * they compute with rows = 1 (they read j -+ 1 only): only the message grows.  EVERY band of a run must declare the
 * same depth, as with the scheme and the count: the neighbours' messages have one size.
 * Errors: a null handle or rows outside {1, 2} GCM_ERR_ARG; any handle but a GCM_PE25D band GCM_ERR_UNSUPPORTED;
 * a call after send or exchange buffers were registered GCM_ERR_STATE, and so is rows = 1 while GCM_TRACER_VANLEER
 * is in force.  A refused call leaves depth, tracers and scheme as they were.
 * gcm_band_tracer_rows: the depth in force (a single domain and other models: 0).                          */
int gcm_set_band_tracer_rows(gcm_handle *h, int rows);
int gcm_band_tracer_rows(const gcm_handle *h);
/* The monitor of the passive tracers of GCM_PE25D, reduced on the device (fp64 and fp32 handles, single domains and
 * latitude bands): one record of GCM_TRACER_STATS_WORDS doubles per tracer, in tracer order, and -- with_q != 0 -- one
 * more for q, last (with n = 0 too):
 *   min, max, mass = sum_{k,j,i} c p dsig_k, air = sum_{k,j,i} p dsig_k, the number of cells < 0, the number of NaN cells.
 * which = 0: the current tracers, with p and q of the current state (gcm_get_state); 1: those of the last predictor
 * (GCM_ERR_STATE where gcm_get_tracers(which = 1) gives it) with p and q of the predicted state (q: GCM_ERR_STATE
 * where gcm_get_star gives it; with n = 0 and with_q that is the only rule).  mass is the quantity the flux-form
 * update conserves under every scheme: the UNWEIGHTED sum -- the meridional flux divergence carries 1 / dy only and
 * telescopes without a row weight, so an area-weighted sum drifts -- and mass / air is the mass-weighted mean mixing
 * ratio; air is the same number in every record of a call.  Values are widened exactly from the storage type, dsig
 * is the float64 table of gcm_config, products and sums are float64; partial sums combine in a fixed order (no
 * atomics), so a call repeated on the same state returns the same bits.  min and max are NaN when the field holds a
 * NaN (np.min / np.max), mass is then whatever the arithmetic gives; -0.0 and NaN are not counted as negative.
 * The sums cover the handle's own rows: a band's ghost rows are never read, so the call is valid right after a
 * step, and the bands' records merge into the global one (min of mins, max of maxes, sums).  The call includes the
 * tracer stream first, as gcm_get_tracers does, synchronises once and changes nothing a later step reads; 48 bytes
 * a record come back.  cap = the doubles `out` holds: fewer than GCM_TRACER_STATS_WORDS (n + (with_q ? 1 : 0))
 * GCM_ERR_ARG (nothing written); n = 0 without q writes nothing and returns GCM_OK.  A null handle or `out`:
 * GCM_ERR_ARG; other models: GCM_ERR_UNSUPPORTED.                                                            */
#define GCM_TRACER_STATS_WORDS 6
int gcm_tracer_stats(gcm_handle *h, int which, int with_q, double *out, int cap);
/* Forcing of one passive tracer of GCM_PE25D: a uniform source, a decay, an emission field and cells held at a value,
 * applied on the device once per Matsuno step right behind the corrector (an operator split, as the solar step is for
 * theta).  The corrector writes its new current value c into each own cell of a forced tracer; the forcing then
 * computes, in the handle's real type T and with every operation rounded on its own (no fused multiply-add):
 *   c1 = c + dt * (source + e)      e = emission at the cell, or T(0) without an emission field
 *   c2 = c1 * fac                   fac = T(exp(-decay * dt)), exp evaluated on the host in double
 *   c  = pinned ? T(pin_value) : c2 pinned: pin_mask is given and non-zero at the cell
 * dt is the stage's dt in T, as the tracer kernel receives it (the exponent takes that value widened to double); fac
 * follows a change of dt.  source and emission are in units of c per second, decay in 1 / s.  emission and pin_mask
 * are host arrays [L][H][W] (a band: its own rows), copied to the device at the call: the caller's arrays are free
 * afterwards.  Without a pin_mask pin_value is not used.
 * The predictor's (star) tracers are never forced: gcm_get_tracers(which = 1) stays the plain predictor, and so do the
 * predicted rows a band sends; the corrected edge rows are forced before they are packed, so a neighbour receives
 * forced values, and no ghost row is ever forced locally.  gcm_set_tracers itself applies nothing: pins take effect
 * from the first step on.  q is never forced.  Only forced tracers cost anything: one launch per corrector launch
 * that reads and writes the forced tracers' own rows (and reads the fields a tracer registered); with no forcing
 * registered nothing is launched and every result and timing is as before.
 * gcm_set_tracer_forcing: registers (replaces) the forcing of tracer `tracer`; f == NULL clears it, tracer == -1
 * with f == NULL clears every tracer's.  It includes the tracer stream first, as gcm_set_tracers does.  The forcing
 * survives gcm_set_tracers with an unchanged count, gcm_set_tracer_scheme and gcm_set_state; it is dropped by
 * gcm_set_tracers with another count (0 included) and by any reallocation of gcm_set_band_tracers or
 * gcm_set_band_tracer_rows.  Errors: a null handle, a tracer outside [0, gcm_tracer_count) (tracer == -1 with a
 * record too), a non-finite source, decay or pin_value, decay < 0: GCM_ERR_ARG; other models: GCM_ERR_UNSUPPORTED.
 * A refused call changes nothing.
 * gcm_tracer_forced: 1 where tracer `tracer` has a forcing registered, else 0; a null handle or a tracer outside
 * [0, gcm_tracer_count): GCM_ERR_ARG; other models: GCM_ERR_UNSUPPORTED.                                      */
typedef struct gcm_tracer_forcing {
    double source, decay, pin_value;
    const double *emission;          /* host [L][H][W] or NULL */
    const unsigned char *pin_mask;   /* host [L][H][W] or NULL */
} gcm_tracer_forcing;
int gcm_set_tracer_forcing(gcm_handle *h, int tracer, const gcm_tracer_forcing *f);
int gcm_tracer_forced(const gcm_handle *h, int tracer);
/* Implicit vertical mixing of one passive tracer of GCM_PE25D: backward-Euler diffusion of the mixing ratio in sigma,
 * zero flux at the top and the bottom, with a horizontally uniform profile K[m], m = 0 .. L - 2: the diffusivity at the
 * interface between levels m and m + 1 in sigma^2 / s (float64, finite, >= 0).  Applied on the device once per Matsuno
 * step, behind the corrector and IN FRONT OF the forcing above (corrector, mixing, forcing): pinned cells hold their
 * value at the end of a step, and what a surface emission adds in step n is mixed in step n + 1.  Pins are not
 * boundary conditions of the solve.
 * The coefficients are float64, computed on the host, every operation rounded on its own, in this order (dsig: the
 * table of gcm_config; dtd: the stage's dt in the handle's real type T, widened to double, as for the forcing's fac):
 *   a[-1] = a[L-1] = 0;   a[m] = dtd * K[m] / (0.5 * (dsig[m] + dsig[m+1]))
 *   lo[k] = a[k-1] / dsig[k];   up[k] = a[k] / dsig[k];   d = 1.0 + lo[k] + up[k]
 *   w[0]  = 1.0 / d;            w[k] = 1.0 / (d - lo[k] * g[k-1])   (k >= 1)
 *   g[k]  = up[k] * w[k]
 * lo, w and g are then rounded to T, and each own column c[0 .. L) of a mixed tracer is solved in T, again with every
 * operation rounded on its own (no fused multiply-add):
 *   y[0] = c[0] * w[0];       y[k] = (c[k] + lo[k] * y[k-1]) * w[k]     k = 1 .. L-1
 *   x[L-1] = y[L-1];          x[k] = y[k] + g[k] * x[k+1]               k = L-2 .. 0;      c = x
 * All coefficients are >= 0: a non-negative column stays non-negative.  sum_k c dsig of a column, and with it the
 * monitor's mass, is conserved up to rounding.  Backward Euler is stable for every dt.  An all-zero K is legal and is
 * launched: the identity on finite columns.
 * The predictor's (star) tracers are never mixed, no ghost row is ever mixed locally (a band's corrected edge rows are
 * mixed, then forced, before they are packed), q is never mixed.  Only mixed tracers cost anything: one launch per
 * corrector launch that reads and writes their own rows once; with no mixing registered nothing is launched and every
 * result and timing is as before.  The handle keeps K in float64 and builds the tables in T again when a stage comes
 * with another dt than the one they were built for, not on every step.
 * gcm_set_tracer_mixing: registers (replaces) the profile of tracer `tracer`, nk = L - 1 values; k == NULL clears it,
 * tracer == -1 with k == NULL clears every tracer's.  It includes the tracer stream first, as gcm_set_tracer_forcing
 * does, and has the forcing's life cycle: it survives gcm_set_tracers with an unchanged count, gcm_set_tracer_scheme and
 * gcm_set_state; it is dropped by gcm_set_tracers with another count (0 included) and by any reallocation of
 * gcm_set_band_tracers or gcm_set_band_tracer_rows.  Errors: a null handle, a tracer outside [0, gcm_tracer_count)
 * (tracer == -1 with a k too), nk != L - 1, a non-finite or negative K, L = 1: GCM_ERR_ARG; other models:
 * GCM_ERR_UNSUPPORTED.  A refused call changes nothing.
 * gcm_tracer_mixed: 1 where tracer `tracer` has a profile registered, else 0; errors as gcm_tracer_forced.
 * gcm_tracer_mixing_coeffs: the coefficient routine above on its own, without a handle or a device -- the routine
 * gcm_set_tracer_mixing's launches take their tables from.  lo, w, g [L] are float64, not yet rounded to T.  Errors
 * (GCM_ERR_ARG, message: gcm_last_error(NULL)): L < 2, a null pointer, a non-finite or negative K.              */
int gcm_set_tracer_mixing(gcm_handle *h, int tracer, const double *k, int nk);
int gcm_tracer_mixed(const gcm_handle *h, int tracer);
int gcm_tracer_mixing_coeffs(int L, const double *dsig, const double *k, double dtd,
                             double *lo, double *w, double *g);
/* Convective mixing of the passive tracers of GCM_PE25D on the device, opt-in per tracer, SINGLE DOMAINS ONLY, fp64 and
 * fp32 handles: a tracer that has opted in is pooled in the blocks of the convective adjustment (gcm_set_convect,
 * gcm_convect_step, below), which otherwise leaves every tracer where it was.
 * One column, level k = 0 at the bottom.  The blocks are those the adjustment forms for that column in that application:
 * the same p and theta as they stand just ahead of it, the same kappa_c, the same pooling routine; there is no second
 * criterion.  For every merged block (n > 1) over levels [k0, k0 + n) and every opted-in tracer c, in float64 for
 * either storage type, every operation rounded on its own (no contraction):
 *   D  = dsig[k0];          D  = D  + dsig[k]          k = k0 + 1 .. k0 + n - 1, ascending
 *   Cs = c[k0] * dsig[k0];  Cs = Cs + c[k] * dsig[k]   likewise
 *   c[k] <- Cs / D for every level of the block, rounded once to the storage type.
 * Levels of unmerged blocks, tracers that have not opted in and stable columns are NOT WRITTEN.  p is constant within a
 * column, so the tracer's mass sum c p dsig (gcm_tracer_stats) is conserved up to rounding, and the output lies within
 * the block's input range.  mix_q plays no part.  The order of the two sums is the contract; it is deliberately NOT the
 * merge-tree order in which the adjustment forms Qs and D of a block: a tracer equal to q equals the mixed q (mix_q = 1)
 * to rounding, not to the bit.
 * Order within a step: ... boundary layer, the tracers' convective mixing, the convective adjustment, the moist physics,
 * the sample.  One launch immediately ahead of every launch of the adjustment (the end of a registered step, and
 * gcm_convect_step), on the handle's stream, which first joins the tracers' last stage launches on the other streams;
 * the next stage's tracer launches follow it.  Nothing is launched, joined or recorded when no tracer has opted in or
 * the adjustment is neither registered nor called: a step then queues exactly what it queued.  The predictor's (star)
 * tracers are never mixed.
 * gcm_set_tracer_convect: on != 0 opts tracer `tracer` in, 0 out.  The opt-in has the forcing's life cycle: it survives
 * gcm_set_tracers with an unchanged count, gcm_set_tracer_scheme and gcm_set_state, and is dropped by gcm_set_tracers
 * with another count (0 included).  Errors: a null handle, a tracer outside [0, gcm_tracer_count): GCM_ERR_ARG; other
 * models, a latitude band (bands are not carried yet: gcm_last_error says so) and a handle whose L makes the blocks of a
 * wave exceed a workgroup's LDS (as gcm_set_convect): GCM_ERR_UNSUPPORTED.  A refused call changes nothing.
 * gcm_tracer_convected: 1 where tracer `tracer` has opted in, else 0; errors as gcm_tracer_forced.
 * gcm_convect_tracer_columns: the pooling and the two sums above on their own, on the host, without a handle or a device
 * -- the routines the kernel calls, compiled for the host, as gcm_convect_columns -- over ncol columns y, w, c [ncol][L]
 * (the adjustment's compared value and weight, the tracer) with dsig [L].  c_out [ncol][L] receives the mixed tracer
 * (levels of unmerged blocks are copied), nblk [ncol][L] the size n of each level's block and may be NULL.  Errors
 * (GCM_ERR_ARG, message: gcm_last_error(NULL)): ncol < 0, L < 1, a missing array.                                  */
int gcm_set_tracer_convect(gcm_handle *h, int tracer, int on);
int gcm_tracer_convected(const gcm_handle *h, int tracer);
int gcm_convect_tracer_columns(int ncol, int L, const double *y, const double *w, const double *dsig, const double *c,
                               double *c_out, int *nblk);

/* Diagnostics the reference's drivers evaluate on the host every step
 * (SURVEY.md 8f-1); computed by device reductions, result copied to *out. */
typedef enum {
    GCM_DIAG_ANY_NAN = 0,   /* np.isnan(u).any() watch            matsuno_c_grid.py:184-187     */
    GCM_DIAG_MAX_U = 1,     /* np.max(u)                          constants.py:111-112          */
    GCM_DIAG_MEAN_P = 2,    /* np.mean(p)                         constants.py:111-112          */
    GCM_DIAG_SUM_P = 3,     /* conservation check                                                */
    GCM_DIAG_MIN_U = 4, GCM_DIAG_MAX_V = 5, GCM_DIAG_MIN_V = 6, /* STATS, no_limits_2_5d.py:85-88 */
    /* get_total_variation(field) = sum |q - roll(q, -1, 0)|  (constants.py:105-108), the monitor
     * run_2d_with_ft evaluates every step (two_d.py:334-338).  Axis 0 of the REFERENCE layout: rows
     * j for 2-D fields, levels k for the 3-D fields of GCM_PE25D.  On a latitude band the last row
     * is differenced against the south ghost row, which must belong to the CURRENT state: a 2-D band
     * exchanges before a step, so after one the call fails with GCM_ERR_STATE until the ghost rows
     * have been exchanged again (gcm_halo_pack2 / exchange / gcm_halo_unpack2); the band sums then
     * add up to the global figure.                                                                */
    GCM_DIAG_TV_P = 7, GCM_DIAG_TV_U = 8, GCM_DIAG_TV_V = 9, GCM_DIAG_TV_T = 10, GCM_DIAG_TV_Q = 11
} gcm_diag_kind;
int gcm_diag(gcm_handle *h, int kind, double *out);
int gcm_diag_members(gcm_handle *h, int kind, double *out, int n);   /* one value per member, see gcm_members */
/* The reductions of constants.py for callers that hold no handle: a host float64 array viewed as
 * [n_axis][n_inner] -> out3 = { get_total_variation (sum |x - roll(x, -1, 0)|, constants.py:105-108),
 * max x, mean x (the two reductions of courant_number, :111-112) }; a NaN anywhere in x makes all
 * three NaN, as np.max / np.mean / np.sum do.  Errors: gcm_last_error(NULL).                     */
int gcm_array_stats(const double *x, long n_axis, long n_inner, double *out3);
/* The whole STATS record of full_timestep (no_limits_2_5d.py:85-91) by ONE launch and ONE
 * synchronisation (GCM_PE25D, fp64, single band): out9 = u_max, u_min, v_max, v_min, ke, ate, geo,
 * total (calc_energy, :35-60; `area` as gcm_energy), the number of cells where u or v is NaN.
 * The extrema are np.max / np.min of each field on its own (:85-88): a NaN in u makes u_max and
 * u_min NaN and leaves v_max and v_min alone, and the other way round.                           */
int gcm_stats(gcm_handle *h, const double *area, int area_len, double *out9);
/* calc_energy(p,u,v,t,q,g,geom) -> out4 = (ke, ate, geo, total) in J, no_limits_2_5d.py:35-60
 * (GCM_PE25D).  `area` is geom.area; the reference broadcasts its (H,) array against the LAST
 * axis (:49), so area_len must be W (== H) or 1 -- reproduced, not fixed.                      */
int gcm_energy(gcm_handle *h, const double *area, int area_len, double *out4);

/* Column physics next to the dynamics (GCM_PE25D).  The ground temperature
 * gt[H][W] (GroundVars.gt, no_limits_2_5d.py:143) lives in the handle.  `lat` [global_height]
 * and `lon` [W] are geom.lat / geom.long in radians; `utc` in seconds.
 *   gcm_grey_radiation  grey_solar.basic_grey_radiation(p,tp,tt,g,t_lw,t_sw,albedo,utc,geom)
 *                       -> dTdt [L][H][W], dt_ground [H][W] (either may be NULL)  grey_solar.py:358-563
 *   gcm_solar_step      no_limits_2_5d.solar_timestep: theta and gt advanced in place by dt
 *                       (the reference passes t_lw = 0.1, t_sw = 0.9, albedo = 0.3)  no_limits_2_5d.py:66-75
 * Accepted by these two, by gcm_set_physics and by gcm_grey_radiation_tables: t_lw and t_sw, the transmissivities of the
 * whole column, in (0, 1] and large enough that no level's share t^dsig[k] rounds to 0 (the level tables divide by it:
 * t_lw = 0 gives 0 / 0 in the reference's own formula); albedo in [0, 1]; utc and dt finite.  Anything else, NaN
 * included, is GCM_ERR_ARG, and the refused call changes nothing: state, ground temperature, registration, clock and the
 * level tables in place stay.  The kernel's arithmetic and every table it reads are float64 on either handle: an fp32
 * handle differs from an fp64 one by the rounding of what it stores (p, theta, dTdt, dt_ground), not by its levels.
 *   gcm_grey_radiation_tables  (no handle, no device) the level tables the kernel reads for (t_lw, t_sw) on the levels
 *                       dsig[L], sig[L], exactly as they are uploaded: out[6][L] = the levels' long-wave and short-wave
 *                       transmissivities t^dsig, the short-wave product from the top down to the level, the long-wave
 *                       product from the bottom up to the level over the level's own, (1 - tsw) csw / tsw, and
 *                       sig^kappa (formed in extended precision); nout >= 6 L doubles in out       grey_solar.py:323-333 */
/* low_pass.arakawa_1977(q, geom) (low_pass.py:41-78) on its own, GCM_PE25D handles: the zonal Fourier
 * damping of nlev <= layers levels of a field on the handle's grid, host [nlev][H][W] float64 in and
 * out (may alias).  Rows are filtered with the multiplier of their global latitude.              */
int gcm_polar_filter(gcm_handle *h, int nlev, const double *in, double *out);
/* Parity tap (GCM_PE25D, single band): the intermediates of the LAST gcm_half_step as the stage kernels
 * themselves left them in the handle -- not a recomputation -- so that a mistake inside K1 / K2 / K3 shows
 * as a wrong intermediate, not only as a wrong stage output.  Host float64, reference layouts.
 *   GCM_INT_SPU   [L][H][W]  spu = arakawa_1977(calc_pu(sp, su))                 dynamics.py:186-190
 *   GCM_INT_PIT   [H][W]     pit = sum_k conv (from the 2-D column sums)         dynamics.py:35-40
 *   GCM_INT_PN    [H][W]     p_n = p - pit dt                                    dynamics.py:194
 *   GCM_INT_PHI   [L][H][W]  compute_geopotential: the stored anchors on the even levels, the odd levels
 *                            rebuilt from them exactly as K3 and K4 do (phi_up)  dynamics.py:111-143
 *   GCM_INT_PGFU  [L][H][W]  arakawa_1977(pgu + phiu)                            dynamics.py:147-171,203      */
typedef enum { GCM_INT_SPU = 0, GCM_INT_PIT = 1, GCM_INT_PN = 2, GCM_INT_PHI = 3, GCM_INT_PGFU = 4 } gcm_intermediate;
int gcm_get_intermediate(gcm_handle *h, int kind, double *out);
int gcm_set_ground(gcm_handle *h, const double *gt);
int gcm_get_ground(gcm_handle *h, double *gt);
int gcm_grey_radiation(gcm_handle *h, double utc, double t_lw, double t_sw, double albedo,
                       const double *lat, const double *lon, double *dTdt, double *dt_ground);
int gcm_solar_step(gcm_handle *h, double dt, double utc, double t_lw, double t_sw, double albedo,
                   const double *lat, const double *lon);
int gcm_grey_radiation_tables(int L, const double *dsig, const double *sig, double t_lw, double t_sw, double *out, int nout);
/* The column physics as the second phase of every step (BASELINE configs[4]: dynamics + solar_timestep;
 * the loop of no_limits_2_5d.run_model, :229-234, with the physics the reference keeps below
 * full_timestep's early return, :94-96).  After gcm_set_physics every step taken by gcm_step and
 * gcm_band_run is  matsuno_timestep(dt)  followed by  solar_timestep(t, p, g, dt, utc, geom)  and
 * utc += dt  (:231).  On a latitude band (nranks > 1) the ghost rows are radiated LOCALLY -- the kernel
 * is column-local, so no third exchange per step is needed: the ghost rows of the ground temperature
 * travel with every ghost-row message (gcm_halo_bytes counts them; pack / unpack move them), the ghost
 * rows of theta that the post-corrector exchange delivers are advanced by the same kernel with the
 * neighbour's own inputs, and so hold the neighbour's own bits.  An explicit gcm_solar_step on a band
 * does the same (own rows and ghost rows), for callers that drive the exchange themselves; the ghost
 * rows of the current state must then be current (the post-corrector exchange unpacked).
 * `lat` [global_height] and `lon` [width] are copied.  NULL switches the physics off.          */
typedef struct {
    double utc;                  /* seconds; advanced by dt after every step                  */
    double t_lw, t_sw, albedo;   /* the reference passes 0.1, 0.9, 0.3  no_limits_2_5d.py:69  */
    const double *lat, *lon;     /* geom.lat [global_height], geom.long [width], radians      */
} gcm_physics;
int gcm_set_physics(gcm_handle *h, const gcm_physics *ph);
int gcm_get_utc(gcm_handle *h, double *utc);   /* the physics clock (GCM_ERR_STATE without gcm_set_physics) */
/* Held & Suarez (1994) forcing of GCM_PE25D on the device: Newtonian relaxation of theta towards a prescribed
 * equilibrium and Rayleigh friction of the low-level winds, backward Euler, one launch per step (fp64 and fp32 handles,
 * single domains and latitude bands).  State: p [H][W] in Pa (surface pressure minus ptop), t = theta, u, v [L][H][W];
 * tables: sig[k] (the mid-level sigma of gcm_config), ptop, lat[j] in radians over the GLOBAL height (a band uses its
 * row offset, as gcm_set_physics does).  P0 = 1e5 Pa and kappa = Rd / Cp are the model's own (constants.py:31,28), not
 * parameters: theta <-> T must agree with the Exner function of the dynamics.
 * Host tables, float64, every operation rounded on its own (gcm_held_suarez_tables):
 *   r[k]     = max(0, (sig[k] - sigma_b) / (1 - sigma_b))
 *   fu[k]    = 1 / (1 + (dt k_f) r[k])
 *   c2[j]    = cos(lat[j])^2;   s2[j] = sin(lat[j])^2
 *   kt[k][j] = k_a + (((k_s - k_a) r[k]) c2[j]) c2[j]
 * r takes the model's own sigma of the level: with ptop = 0, the reference's geometry, that is exactly Held-Suarez's
 * p / p_s; with ptop != 0 it is this build's choice, which keeps the friction a function of the level alone, so that u
 * and v at their C-grid half points need no pressure and no row beyond the ghost rows.
 * Update, float64 arithmetic for either storage type (as the radiation kernel), the result rounded once to it:
 *   levels with r[k] > 0:  u <- u fu[k],  v <- v fu[k];  levels with r[k] = 0 are neither read nor written
 *   p_lev    = sig[k] p[j][i] + ptop
 *   theta_eq = max(T_min (P0 / p_lev)^kappa,  T_0 - dT_y s2[j] - (dtheta_z ln(p_lev / P0)) c2[j])
 *   theta   <- (theta + (dt kt[k][j]) theta_eq) / (1 + dt kt[k][j])
 * Backward Euler: stable for every dt, theta moves monotonically towards theta_eq, |u| never grows.  p, q, the tracers
 * and the ground temperature are untouched.  The device takes (P0 / p_lev)^kappa from the kernels' own Exner routine
 * and multiplies by the host's 1 / (1 + dt kt): theta agrees with the formula within the 1e-10 of the parity tests,
 * u and v (one float64 product with the routine's own table) bit for bit.
 * gcm_set_held_suarez: the forcing as a phase of every step taken by gcm_step and gcm_band_run: the Matsuno step, then
 * solar_timestep where gcm_set_physics is on, then this.  gcm_half_step never applies it (as it never applies the solar
 * step): the predicted (star) state is never forced.  On a latitude band the ghost rows of theta, u, v that the
 * post-corrector exchange delivers are forced LOCALLY (the kernel is column-local and takes the latitude of the global
 * row: the neighbour's own inputs, the neighbour's own bits), the packed edge rows leave unforced: no third exchange,
 * the message format is unchanged.  `lat` [global_height] is copied; NULL switches the forcing off.  Errors, checked in
 * the call: a null handle GCM_ERR_ARG; other models GCM_ERR_UNSUPPORTED; a non-finite number, k_f, k_a or k_s < 0,
 * sigma_b outside [0, 1), a null `lat`: GCM_ERR_ARG.  A refused call changes nothing.  Without a registration nothing
 * is launched and every result and timing is as before.  The handle keeps the parameters and builds the tables again
 * when a step comes with another dt, not on every step.
 * gcm_held_suarez_on: 1 where a forcing is registered, else 0 (other models: 0; a null handle GCM_ERR_ARG).
 * gcm_held_suarez_step: the same kernel once, in place on the current state (what gcm_solar_step is to
 * gcm_set_physics).  On a band it advances own rows and ghost rows: the ghost rows of the current state must be
 * current, as for gcm_solar_step.
 * gcm_held_suarez_tables: the table routine above on its own, without a handle or a device -- the routine the launches
 * take their tables from.  fu [L], kt [L][nlat], s2, c2 [nlat].  Errors (GCM_ERR_ARG, message: gcm_last_error(NULL)):
 * L or nlat < 1, a null pointer, a non-finite dt, sig or lat, the parameter errors above.                       */
typedef struct {
    double k_f, k_a, k_s;        /* 1 / s: friction, relaxation aloft, relaxation at the surface of the tropics */
    double sigma_b;              /* top of the boundary layer                                  */
    double dT_y, dtheta_z;       /* K: equator-to-pole difference, static stability            */
    double T_0, T_min;           /* K: surface equilibrium at the equator, stratosphere        */
    const double *lat;           /* geom.lat [global_height], radians                          */
} gcm_held_suarez;
int gcm_set_held_suarez(gcm_handle *h, const gcm_held_suarez *hs);
int gcm_held_suarez_on(const gcm_handle *h);
int gcm_held_suarez_step(gcm_handle *h, double dt, const gcm_held_suarez *hs);
int gcm_held_suarez_tables(int L, const double *sig, int nlat, const double *lat, const gcm_held_suarez *hs, double dt,
                           double *fu, double *kt, double *s2, double *c2);
/* Moist physics of GCM_PE25D on the device: large-scale condensation of the specific humidity q with latent heating of
 * theta and immediate precipitation (the saturation adjustment of Reed & Jablonowski's simple physics and of Thatcher &
 * Jablonowski (2016)'s moist Held-Suarez test, on the model's own saturation formula), and optionally a moisture source
 * at the level next to the surface.  One launch per step, fp64 and fp32 handles, single domains and latitude bands.
 * The reference has nothing of the kind (its evaporation.py is empty, humidity.py serves the initial field only): this
 * is an addition.  State: p [H][W] in Pa (surface pressure minus ptop), t = theta, q [L][H][W]; tables: sig[k], dsig[k].
 * Constants: Rd = 287, Rv = 461, Cp = 1004, G = 9.8, P0 = 1e5, kappa = Rd / Cp are the model's own (constants.py); eps = Rd / Rv.
 * Arithmetic per cell (k, j, i), float64 for either storage type, every operation rounded on its own (no contraction),
 * the result rounded once to the storage type:
 *   p_lev = sig[k] p + ptop;   Pi = (p_lev / P0)^kappa from the kernels' own Exner routine;   T = theta Pi
 *   tc = T - 273.15;   a = 18.678 - tc / 234.5;   b = tc / (257.14 + tc)
 *   e_s = (0.61121 * 1000.0) exp(a b)                      humidity.saturation_vapor_pressure, the Buck equation
 *   the cell CAN SATURATE iff e_s < p_lev; then
 *     den  = p_lev - (1 - eps) e_s;   q_s = (eps e_s) / den                      = humidity.rh_to_mmr(1, p_lev, T)
 *     dlne = (a * 257.14) / (257.14 + tc)^2 - tc / (234.5 (257.14 + tc))         d ln e_s / dT
 *     dq_s = (q_s (p_lev / den)) dlne                                            d q_s / dT at constant p_lev
 *   otherwise (warm air at low pressure: the top levels of an isothermal column) both processes leave the cell alone.
 *   Condensation, where the cell can saturate and q > q_s:
 *     C = (q - q_s) / (1 + (Lv / Cp) dq_s);   q <- q - C;   theta <- theta + ((Lv / Cp) C) / Pi
 *   One linearised step.  q_s is convex in T, so the step never overshoots: the cell ends at or just below saturation at
 *   its new temperature.  The undershoot is of second order in the excess: for a cell that started 40 % supersaturated it is 3-5 %
 *   of q_s at 300 K, 2-3 % at 285 K and under 0.3 % at 250 K; for one that started 0.1 % over, 4e-7 or less.  A second
 *   application condenses nothing (float64).  Cells that do not condense are not
 *   written.  Cp T + Lv q of the cell is unchanged.
 *   Precipitation of the column, kg / m^2 per application:  P = sum_k C_k ((dsig[k] p) / G), k = 0, 1, .., L - 1 in that
 *   order, from 0.0.  The condensate leaves the column at once.
 *   Evaporation, only with tau_e > 0, on the one level kb with the largest sig (k = 0 in the product's geometries),
 *   behind that level's condensation and with its updated T = theta_new Pi (theta_new in float64):
 *     q_eq = rh_s q_s(T, p_lev);   x = dt / tau_e
 *     where the cell can saturate and q_eq > q:  q_new = (q + x q_eq) / (1 + x);  E = (q_new - q) ((dsig[kb] p) / G);  q <- q_new
 *   dt is taken as given: only a non-finite dt is refused, and the properties below are those of dt >= 0.
 *   Backward Euler and one-sided: q never exceeds q_eq and never decreases.  The heat comes from the surface: theta is
 *   not changed.  p, u, v, the tracers and the ground temperature are untouched.
 * Accumulators in the handle, allocated by gcm_set_moist, own rows only: precip [H][W] and evap [H][W], float64, kg / m^2;
 * seconds (the sum of dt) and nsteps.  One writer per word and launch, no atomics: the same state gives the same bits,
 * and a band's rows hold the bits of the same rows of the single domain.
 * gcm_set_moist: the phase as part of every step taken by gcm_step and gcm_band_run: the Matsuno step, solar_timestep
 * where gcm_set_physics is on, the Held-Suarez forcing where registered, the boundary layer where registered
 * (gcm_set_boundary_layer), the convective adjustment where registered (gcm_set_convect), then this, then the
 * climatology's sample.
 * gcm_half_step and gcm_step_phase never apply it.  On a latitude band the ghost rows of theta and q that the
 * post-corrector exchange delivers are adjusted LOCALLY (column-local kernel, the neighbour's own inputs, the neighbour's
 * own bits) and add to no sum; the packed edge rows leave unadjusted: no third exchange, the message format and
 * gcm_halo_bytes are unchanged.  NULL switches the phase off and frees the accumulators; registering again resets them.
 * Without a registration nothing is launched and every result and timing is as before.
 * gcm_moist_on: 1 where the phase is registered, else 0 (other models: 0; a null handle GCM_ERR_ARG).
 * gcm_moist_step: the same kernel once, in place on the current state (what gcm_held_suarez_step is to
 * gcm_set_held_suarez).  With a registration it adds to the accumulators, to seconds and to nsteps; without one the sums
 * of the call are dropped.  On a band it covers own rows and ghost rows: the ghost rows must be current.
 * gcm_get_moist synchronises the handle's stream once; any pointer may be NULL.  gcm_put_moist uploads sums and counters
 * (restarts): both arrays are required, seconds finite and >= 0, nsteps >= 0.  gcm_moist_reset zeroes all four.
 * gcm_moist_saturation: the saturation routine above on its own, on the host, without a handle or a device -- the one
 * routine the kernel calls, compiled for the host.  q_s, dq_s, can [n], any of them may be NULL; where can = 0, q_s and
 * dq_s are 0.
 * Errors, all checked in the call; a refused call changes nothing.  GCM_ERR_ARG: a null handle, a non-finite parameter,
 * Lv <= 0, tau_e < 0, rh_s outside (0, 1], a non-finite dt.  GCM_ERR_UNSUPPORTED: other models.  GCM_ERR_STATE: get,
 * put or reset without a registration.                                                                           */
typedef struct {
    double Lv;                   /* J / kg: latent heat of vaporisation (2.5e6)                 */
    double tau_e;                /* s: evaporation time scale; 0: no evaporation                */
    double rh_s;                 /* target relative humidity of the lowest level, (0, 1]        */
} gcm_moist;
int gcm_set_moist(gcm_handle *h, const gcm_moist *mo);
int gcm_moist_on(const gcm_handle *h);
int gcm_moist_step(gcm_handle *h, double dt, const gcm_moist *mo);
int gcm_get_moist(gcm_handle *h, double *precip, double *evap, double *seconds, int64_t *nsteps);
int gcm_put_moist(gcm_handle *h, const double *precip, const double *evap, double seconds, int64_t nsteps);
int gcm_moist_reset(gcm_handle *h);
int gcm_moist_saturation(int n, const double *T, const double *p_lev, double *q_s, double *dq_s, int *can);
/* Convective adjustment of GCM_PE25D on the device: every column's theta, and optionally q, is mixed wherever it is
 * statically unstable against a neutral profile, at constant column enthalpy and column water (the dry adjustment, and
 * with a critical lapse rate the adjustment of Manabe & Strickler (1964)).  One launch per step, fp64 and fp32 handles,
 * single domains and latitude bands.  The reference has nothing of the kind: this is an addition.  State: p [H][W] in Pa
 * (surface pressure minus ptop), t = theta, q [L][H][W]; tables: sig[k], dsig[k]; level k = 0 is the bottom.
 * The one parameter kappa_c chooses the neutral profile: kappa_c = 0 is the dry adjustment, neutral where theta is
 * constant; kappa_c = Rd gamma / G adjusts to the critical lapse rate gamma = -dT/dz (K / m; 6.5e-3 gives 0.19036),
 * neutral where T is proportional to p_lev^kappa_c.
 * Arithmetic, float64 for either storage type, every operation rounded on its own (no contraction), the result rounded
 * once to the storage type.  Per cell (k, j, i):
 *   p_lev = sig[k] p + ptop;   Pi = (p_lev / P0)^kappa from the kernels' own Exner routine
 *   r = 1 where kappa_c = 0, else r = exp((kappa_c - kappa) log(p_lev / P0))
 *   the compared value  y = theta / r  (kappa_c = 0: theta itself, no operation on it)
 *   the weight          w = (Pi r) dsig[k],  so that sum_k y w = sum_k T dsig, the column's enthalpy up to Cp p / G
 * Per column, pool adjacent violators from the bottom up:
 *   for k = 0 .. L - 1: push the block (S = w y, Wt = w, Qs = q dsig[k], D = dsig[k], n = 1, value = y);
 *     while there are two blocks and top.value < below.value (strict; a NaN compares false): pop the top into the one
 *     below,  S = below.S + top.S, likewise Wt, Qs, D and n, in that operand order, then value = S / Wt
 *   afterwards every level of a block with n > 1:  theta <- value r  (kappa_c = 0: value);  with mix_q: q <- Qs / D
 *   blocks with n = 1 are NOT WRITTEN: a stable column, and the stable part of any column, keeps its bits.
 * Both loops are bounded by L.  The result is the weighted isotonic regression of y, the exact limit of the classic
 * pairwise adjustment sweeps: no iteration count, no tolerance.  y comes out non-decreasing in k; sum_k T dsig and
 * sum_k q dsig of the column are conserved to rounding; a second application changes no bit where kappa_c = 0.
 * p, u, v, the ground temperature and the tracers are untouched (a tracer that has opted in through
 * gcm_set_tracer_convect is mixed in the same blocks by a launch of its own ahead of this one).
 * Accumulators in the handle, allocated by gcm_set_convect, own rows only: count [H][W] and levels [H][W], float64;
 * an application adds 1 to count where the column had a merged block and sum of n over its merged blocks to levels.
 * seconds (the sum of the registered steps' dt) and nsteps (the applications).  One writer per word and launch, no atomics.
 * gcm_set_convect: the phase as part of every step taken by gcm_step and gcm_band_run: the Matsuno step, solar_timestep
 * where gcm_set_physics is on, the Held-Suarez forcing where registered, the boundary layer where registered
 * (gcm_set_boundary_layer), then this, then the moist physics where
 * registered (which condenses what the mixing left supersaturated), then the climatology's sample.  gcm_half_step and
 * gcm_step_phase never apply it.  On a latitude band the ghost rows of theta and q that the post-corrector exchange
 * delivers are adjusted LOCALLY (column-local kernel, the neighbour's own inputs, the neighbour's own bits) and add to no
 * sum; the packed edge rows leave unadjusted: no third exchange, the message format and gcm_halo_bytes are unchanged.
 * NULL switches the phase off and frees the accumulators; registering again resets them.  Without a registration nothing
 * is launched and every result and timing is as before.
 * gcm_convect_on: 1 where the phase is registered, else 0 (other models: 0; a null handle GCM_ERR_ARG).
 * gcm_convect_step: the same kernel once, in place on the current state.  It takes no dt: the adjustment is
 * instantaneous.  With a registration it adds to count, levels and nsteps (and nothing to seconds); without one the counts
 * of the call are dropped.  On a band it covers own rows and ghost rows: the ghost rows must be current.
 * gcm_get_convect synchronises the handle's stream once; any pointer may be NULL.  gcm_put_convect uploads sums and
 * counters (restarts): both arrays are required, seconds finite and >= 0, nsteps >= 0.  gcm_convect_reset zeroes all four.
 * gcm_convect_columns: the pooling above on its own, on the host, without a handle or a device -- the one routine the
 * kernel calls, compiled for the host -- over ncol columns y, w, q [ncol][L] with dsig [L].  y_out and q_out [ncol][L]
 * receive the adjusted y and q (q unchanged without mix_q; levels of unmerged blocks are copied), nblock [ncol][L] the
 * size n of each level's block; any of the three may be NULL.
 * The kernel keeps a column's blocks in LDS, 44 bytes per level and lane of a one-wave workgroup.
 * Errors, all checked in the call; a refused call changes nothing.  GCM_ERR_ARG: a null handle, no parameters, kappa_c
 * not finite or outside [0, 1), mix_q not 0 or 1; the probe: ncol < 0, L < 1, a missing input.  GCM_ERR_UNSUPPORTED: other
 * models, and a handle whose L makes the blocks of a wave exceed a workgroup's LDS (L = 40 fits; 160 KB hold L = 57).
 * GCM_ERR_STATE: get, put or reset without a registration.                                                         */
typedef struct {
    double kappa_c;              /* Rd gamma / G of the neutral profile, [0, 1); 0: dry adjustment */
    int32_t mix_q;               /* 1: q of a merged block becomes its mass-weighted mean; 0: q is left alone */
} gcm_convect;
int gcm_set_convect(gcm_handle *h, const gcm_convect *cv);
int gcm_convect_on(const gcm_handle *h);
int gcm_convect_step(gcm_handle *h, const gcm_convect *cv);
int gcm_get_convect(gcm_handle *h, double *count, double *levels, double *seconds, int64_t *nsteps);
int gcm_put_convect(gcm_handle *h, const double *count, const double *levels, double seconds, int64_t nsteps);
int gcm_convect_reset(gcm_handle *h);
int gcm_convect_columns(int ncol, int L, const double *y, const double *w, const double *q, const double *dsig, int mix_q,
                        double *y_out, double *q_out, int32_t *nblock);
/* Betts-Miller convection of GCM_PE25D on the device: the simplified Betts-Miller scheme of Frierson (2007).  Every column
 * relaxes, over the time tau, towards the moist adiabat of a parcel lifted from its lowest level and towards the relative
 * humidity rh_bm on that adiabat; what the relaxation takes out of q is the convective precipitation, and the reference
 * temperature is shifted uniformly so that the column's enthalpy is conserved.  One launch per step, fp64 and fp32
 * handles, single domains and latitude bands.  The reference has nothing of the kind: this is an addition.  Only the
 * deep-convection case is built: the paper's shallow-convection closures (for columns whose relaxation would make
 * negative precipitation) and any convective momentum transport are out of scope; such columns are left to the
 * convective adjustment.  State: p [H][W] in Pa (surface pressure minus ptop), t = theta, q [L][H][W]; tables: sig[k],
 * dsig[k]; level k = 0 is the bottom and sig must strictly decrease in k.  Constants as for gcm_moist; lc = Lv / Cp;
 * (q_s, dq_s, can) = the saturation routine of gcm_moist at (T, p), with pd = p / den of that routine.
 * Arithmetic per column, float64 for either storage type, every operation rounded on its own (no contraction), the
 * results rounded once to the storage type.  Per level:  p_lev = sig[k] p + ptop;  Pi = (p_lev / P0)^kappa from the
 * kernels' own Exner routine;  T = theta Pi;  w = (dsig[k] p) / G.
 * 1. The parcel's ascent, k = 0, 1, ..:
 *   k = 0:  T_p = T;  the parcel keeps theta_0 = theta[0] and q_0 = q[0];  s = saturation(T_p, p_lev)
 *   k >= 1, no LCL yet:  T_d = theta_0 Pi;  s = saturation(T_d, p_lev);  T_p = T_d;  where s.q_s <= q_0 (a NaN compares
 *     false) this level is k_lcl and the parcel takes the moist physics' one linearised condensation step:
 *       C = (q_0 - s.q_s) / (1 + lc s.dq_s);  T_p = T_d + lc C;  s = saturation(T_p, p_lev)
 *     (the search starts at level 1: level 0 is where the parcel comes from)
 *   k > k_lcl: the pseudoadiabat of that q_s, dT/dp = slope(T, p) = (kappa T + (lc q_s) pd) / ((1 + lc dq_s) p) -- which is
 *     Cp dT - (Rd T / p) dp + Lv dq_s = 0 -- from (T_p[k-1], p_lev[k-1]) to p_lev by nsub explicit midpoint steps of
 *     h = (p_lev - p_lev[k-1]) / nsub:  T_c = T_p[k-1];  for n = 0 .. nsub - 1:  p_a = p_lev[k-1] + n h;
 *       f_1 = slope(T_c, p_a);  T_m = T_c + (0.5 h) f_1;  p_m = p_a + 0.5 h;  f_2 = slope(T_m, p_m);  T_c = T_c + h f_2
 *     then T_p = T_c;  s = saturation(T_p, p_lev).  The count is fixed: no tolerance, no iteration that depends on data.
 *   Any of these evaluations that cannot saturate ends the ascent below level k.
 * 2. Cloud top.  At every level k >= k_lcl: buoyant = T_p > T (strict; a NaN compares false).  A buoyant level becomes kt;
 *   a level that is not buoyant while there is a kt ends the ascent below it: kt is the top of the first contiguous run of
 *   buoyant levels at or above k_lcl.  A column with no k_lcl or no such run does not convect.
 * 3, 4. Every level the ascent takes (0 .. kt, and the levels it looked at above in vain):  T_ref = T_p;
 *   q_ref = rh_bm s.q_s;  x = dt / tau;  r = x / (1 + x) (backward Euler: stable for every dt >= 0; dt is taken as given,
 *   only a non-finite one is refused);  dq = -r (q - q_ref);  dT = -r (T - T_ref);  running sums from 0.0, in level order:
 *   P = P - dq w;  S = S + dT w;  M = M + w.  P_q, S_T and M_t are P, S and M as they stand behind level kt.
 * 5. Deep convection iff there is a kt and P_q > 0 and S_T > 0.  Then  D = (lc P_q - S_T) / (r M_t)  and for k = 0 .. kt:
 *   theta <- theta + (dT + r D) / Pi;   q <- q + dq.   Every other column is NOT WRITTEN.
 * Properties: sum_k (Cp dT + Lv dq) w = 0 and sum_k dq w = -P_q over the levels written, to rounding; q stays >= 0 (it
 * becomes (1 - r) q + r q_ref); p, u, v, the tracers and the ground temperature are untouched.
 * Accumulators in the handle, allocated by gcm_set_betts_miller, own rows only: precip [H][W], float64, kg / m^2, += P_q,
 * and count [H][W], float64, += 1, for a column that convected; seconds (the sum of dt) and nsteps.  One writer per word
 * and launch, no atomics: the same state gives the same bits, and a band's rows hold the bits of the same rows of the
 * single domain.
 * gcm_set_betts_miller: the phase as part of every step taken by gcm_step and gcm_band_run: the Matsuno step, the
 * horizontal diffusion, solar_timestep, the Held-Suarez forcing, the boundary layer, the convective adjustment, each where
 * registered, then this, then the moist physics where registered (which condenses what the relaxation left
 * supersaturated), then the samples.  gcm_half_step and gcm_step_phase never apply it.  On a latitude band the ghost rows
 * that the step's last exchange delivers are relaxed LOCALLY (column-local kernel, the neighbour's own inputs, the
 * neighbour's own bits) and add to no sum: no further exchange, no opt-in, the message format and gcm_halo_bytes are
 * unchanged; a band with the boundary layer registered takes the phase in the part of the walk behind its third
 * exchange.  NULL switches the phase off and frees the accumulators; registering again resets them.  Without a
 * registration nothing is launched and every result and timing is as before.
 * gcm_betts_miller_on: 1 where the phase is registered, else 0 (other models: 0; a null handle GCM_ERR_ARG).
 * gcm_betts_miller_step: the same kernel once, in place on the current state, with the step dt.  With a registration it
 * adds to the accumulators, to seconds and to nsteps; without one the sums of the call are dropped.  On a band it covers
 * own rows and ghost rows: the ghost rows must be current.
 * gcm_get_betts_miller synchronises the handle's stream once; any pointer may be NULL.  gcm_put_betts_miller uploads sums
 * and counters (restarts): both arrays are required, seconds finite and >= 0, nsteps >= 0.  gcm_betts_miller_reset zeroes
 * all four.
 * gcm_betts_miller_columns: the rule above on its own, on the host, without a handle or a device -- the very routines the
 * kernel calls, compiled for the host -- over ncol columns: p [ncol], theta and q [ncol][L], sig and dsig [L].  theta_out
 * and q_out [ncol][L] receive the columns as the phase leaves them (unchanged where the column did not convect), precip
 * [ncol] P_q or 0, kt [ncol] the cloud top or -1 where the column did not convect, k_lcl [ncol] the LCL's level or -1;
 * any of them may be NULL.  margin [ncol] (may be NULL) is the smallest relative distance of any comparison the column
 * consulted -- |a - b| / max(|a|, |b|) for q_s <= q_0 at every level searched and for T_p > T at every level tested;
 * |P_q| / sum |dq w| and |S_T| / sum |dT w| over levels 0 .. kt for the two signs, where there is a kt -- and +infinity
 * where it consulted none: a column whose margin is far above the rounding of exp keeps its outcome on any device.
 * The kernel parks dT and dq of a column in LDS, 16 bytes per level and lane of a one-wave workgroup, beside the 2 KB
 * Exner table: GCM_BETTS_MILLER_MAX_LEVELS levels fill a workgroup's 160 KB.
 * Errors, all checked in the call; a refused call changes nothing.  GCM_ERR_ARG: a null handle, no parameters, a
 * non-finite parameter or dt, Lv <= 0, tau <= 0, rh_bm outside (0, 1], nsub outside [1, 8]; the probe: ncol < 0, L < 1, a
 * non-finite ptop, a missing input.  GCM_ERR_UNSUPPORTED: other models, L < 2, a sig table that does not strictly
 * decrease, L > GCM_BETTS_MILLER_MAX_LEVELS.  GCM_ERR_STATE: get, put or reset without a registration.              */
#define GCM_BETTS_MILLER_MAX_LEVELS 158
typedef struct {
    double Lv;                   /* J / kg: latent heat of vaporisation (2.5e6)                 */
    double tau;                  /* s: relaxation time, > 0 (7200)                              */
    double rh_bm;                /* relative humidity of the reference profile, (0, 1] (0.7)    */
    int nsub;                    /* midpoint steps per level of the pseudoadiabat, [1, 8] (2)   */
} gcm_betts_miller;
int gcm_set_betts_miller(gcm_handle *h, const gcm_betts_miller *bm);
int gcm_betts_miller_on(const gcm_handle *h);
int gcm_betts_miller_step(gcm_handle *h, double dt, const gcm_betts_miller *bm);
int gcm_get_betts_miller(gcm_handle *h, double *precip, double *count, double *seconds, int64_t *nsteps);
int gcm_put_betts_miller(gcm_handle *h, const double *precip, const double *count, double seconds, int64_t nsteps);
int gcm_betts_miller_reset(gcm_handle *h);
int gcm_betts_miller_columns(int ncol, int L, const double *p, const double *theta, const double *q, const double *sig,
                             const double *dsig, double ptop, double dt, const gcm_betts_miller *bm, double *theta_out,
                             double *q_out, double *precip, int32_t *kt, int32_t *k_lcl, double *margin);
/* Surface fluxes and boundary-layer mixing of GCM_PE25D on the device: bulk exchange of momentum, heat and moisture with a
 * surface of prescribed temperature (the ground temperature of gcm_set_ground: an ocean, it is read and never changed) and
 * the implicit diffusion that carries the fluxes upwards -- the two parts of Reed & Jablonowski (2012)'s simple physics,
 * as used by Thatcher & Jablonowski (2016)'s moist Held-Suarez test, that the moist physics above leaves out.  Two
 * launches per step, fp64 and fp32 handles, SINGLE DOMAINS ONLY.  The reference has nothing of the kind: this is an
 * addition.  State: p [H][W] in Pa (surface pressure minus ptop), u, v, t = theta, q [L][H][W] on the C grid (u between the
 * centres i and i + 1, v between the rows j and j + 1); tables sig[k], dsig[k]; level k = 0 is the bottom.  Constants: Rd,
 * Rv, Cp, G, P0 as for the moist physics.  With this phase on, tau_e of gcm_set_moist should be 0: two moisture sources
 * otherwise.
 * Arithmetic, float64 for either storage type, every operation rounded on its own (no contraction), the result rounded
 * once to the storage type.  Coefficients are explicit, taken from the state at phase entry; the solves are implicit, so
 * the phase is stable for every dt.
 * (A) Centre quantities of the column (j, i); i and j are periodic, as in the dynamics and in the climatology's uc, vc;
 *     T_s is the ground temperature of the cell:
 *   uc = 0.5 (u[0][j][i] + u[0][j][i-1]);   vc = 0.5 (v[0][j][i] + v[0][j-1][i]);   S = sqrt(uc uc + vc vc)
 *   p_s = p + ptop;   p_a = sig[0] p + ptop;   Pi_a = (p_a / P0)^kappa from the kernels' own Exner routine;   T_a = theta[0] Pi_a
 *   z_a = ((Rd / G) (T_a (1 + (Rv / Rd - 1) q[0]))) log(p_s / p_a)
 *   cd  = cd0 + cd1 min(S, v_cap);     r = S / z_a
 *   (q_ss, can_s) = the saturation routine of the moist physics at (T_s, p_s)
 *   interfaces m = 0 .. L-2:   sig_e = sig[m] - 0.5 dsig[m];   p_e = sig_e p + ptop
 *     T_e = 0.5 (theta[m] Pi_m + theta[m+1] Pi_{m+1});   rho_e = p_e / (Rd T_e);   gr = (G rho_e) / p
 *     f = 1 where p_e >= p_pbl, else exp(-(((p_pbl - p_e) / p_strat)^2))
 *     e[m] = (((S z_a) f) (gr gr)) / (0.5 (dsig[m] + dsig[m+1]))
 *   This is dX/dt = (g^2 / p^2) d/dsigma (rho^2 K dX/dsigma) with K = C S z_a f; the factor C is applied per field below.
 * (B) Four column solves, each "surface step on level 0, then diffusion":
 *   field   surface weight x                               target        interface coefficient a[m]
 *   theta   (dt ch) r                                      T_s / Pi_a    (dt ce) e[m]
 *   q       (dt ce) r, 0 where can_s = 0                   q_ss          (dt ce) e[m]
 *   u       dt (0.5 (cd_i r_i + cd_{i+1} r_{i+1}))         0             dt (0.5 (cd_i e_i[m] + cd_{i+1} e_{i+1}[m]))
 *   v       dt (0.5 (cd_j r_j + cd_{j+1} r_{j+1}))         0             dt (0.5 (cd_j e_j[m] + cd_{j+1} e_{j+1}[m]))
 *   X0' = (X[0] + x target) / (1 + x)                       the surface step (two-sided: dew is allowed)
 *   lo[k] = a[k-1] / dsig[k];  up[k] = a[k] / dsig[k]  (a[-1] = a[L-1] = 0);   d = (1 + lo[k]) + up[k]
 *   w[0] = 1 / d;  w[k] = 1 / (d - lo[k] g[k-1]);  g[k] = up[k] w[k]
 *   y[0] = X0' w[0];  y[k] = (X[k] + lo[k] y[k-1]) w[k];     X[L-1] = y[L-1];  X[k] = y[k] + g[k] X[k+1]
 *   The recurrence is the tracer mixing's (gcm_set_tracer_mixing), with float64 coefficients of the column's own.  All
 *   coefficients are >= 0: max |u| and max |v| of a column do not grow, theta and q stay within the range of the column
 *   and the target; sum_k X dsig changes by the surface step alone.  An atmosphere at rest (S = 0) and dt = 0 keep every bit.
 *   p, the tracers and the ground temperature are untouched.
 * Accumulators in the handle, allocated by gcm_set_boundary_layer, every row, with m = (dsig[0] p) / G:
 *   shf [H][W], J / m^2:   shf += ((Cp Pi_a) (theta0' - theta0)) m        evap [H][W], kg / m^2:   evap += (q0' - q0) m
 *   (theta0', q0': the surface step's results in float64); seconds (the sum of dt) and nsteps.  One writer per word and
 *   launch, no atomics.
 * The phase is not column-local: a u- or v-column takes cd, r and e from two neighbouring centre columns.  Every launch is
 * race-free by construction: the first writes cd, r and e of its own column to float64 scratch fields of the handle (two
 * [H][W], one [H][L-1][W]) and solves theta and q of that column, reading u and v, which it does not write; the second
 * solves u and v from the scratch fields and the lane's own column.
 * gcm_set_boundary_layer: the phase as part of every step taken by gcm_step and gcm_end_step: the Matsuno step,
 * solar_timestep where gcm_set_physics is on, the Held-Suarez forcing where registered, then this, then the convective
 * adjustment (which mixes what the heated lowest level made unstable), the moist physics (which condenses what became
 * supersaturated) and the climatology's sample.  gcm_half_step and gcm_step_phase never apply it.  Registration allocates
 * the accumulators and the scratch fields; NULL switches the phase off and frees them; registering again resets the
 * accumulators.  Without a registration nothing is launched and every result and timing is as before.
 * Latitude bands (nranks > 1): the centre quantities of ghost row -2 need v of row -3, and v of ghost row H + 1 needs
 * the centre quantities of row H + 2; neither exists, so the ghost rows cannot be advanced locally to the neighbour's
 * bits, which is how every other phase avoids a third exchange.  A band is therefore refused by default, and takes the
 * phase after gcm_set_band_boundary_layer(h, 1), right after gcm_create and on every band of a run.  The launches then
 * take the band's OWN rows: the first runs over rows [0, H] and forms cd, r and e only on ghost row H (no solve, no
 * store to theta or q, no sum), the second over rows [0, H); j is not periodic, rows j - 1 and j + 1 are the
 * neighbouring rows of the band (scratch: cd, r and e hold H + 1 rows).  They read v of ghost row -1 and every field of
 * ghost row H, which must be current: the post-corrector exchange unpacked, the solar step and the Held-Suarez forcing
 * applied to them.  The ghost rows are not advanced: the edge rows of the current state are exchanged a THIRD time
 * behind the phase, in the message of every other exchange (gcm_halo_pack2 / gcm_halo_unpack2 with no phase pending,
 * the same buffers, gcm_halo_bytes unchanged), which overwrites the ghost rows of u, v, theta and q with the
 * neighbour's own bits.  The convective adjustment and the moist physics then take own rows and ghost rows locally, as
 * ever.  Own rows see the same inputs and the same arithmetic in the same order as the single domain's: the same bits;
 * shf and evap take rows [0, H).  A step of such a band, by gcm_band_run or by the host:
 *   1. the Matsuno step with its two exchanges;
 *   2. solar step and Held-Suarez forcing on own rows and ghost rows;        | gcm_end_step_begin
 *   3. the boundary layer on the own rows;                                   |
 *   4. the third exchange: pack / send and receive / unpack of the current state;
 *   5. convective adjustment and moist physics on own rows and ghost rows;   | gcm_end_step_finish
 *   6. the climatology's sample, then the spectra's; both read v of ghost    |
 *      row -1.                                                              |
 * gcm_band_run queues all six (the exchange and the ghost rows' launches beside the own rows' convective adjustment
 * and moist physics on its second stream).  A host that drives the exchange itself calls gcm_end_step_begin, moves the
 * ghost rows, then gcm_end_step_finish; gcm_end_step on such a band is GCM_ERR_STATE and changes nothing.  The third
 * exchange costs one more message of gcm_halo_bytes per neighbour and step.
 * gcm_set_band_boundary_layer(h, on): GCM_PE25D latitude bands only -- other models, and a single domain with on != 0,
 * GCM_ERR_UNSUPPORTED (a single domain with on = 0: GCM_OK, nothing to do); on = 0 while the phase is registered
 * GCM_ERR_STATE (unregister first); a null handle GCM_ERR_ARG.  A refused call changes nothing.  The opt-in by itself
 * launches nothing and changes no result or timing.  gcm_band_boundary_layer: 1 on a band that has opted in, else 0 (a
 * null handle GCM_ERR_ARG).
 * gcm_boundary_layer_on: 1 where the phase is registered, else 0 (other models: 0; a null handle GCM_ERR_ARG).
 * gcm_boundary_layer_step: the same launches once, in place on the current state.  With a registration it adds to the
 * accumulators, to seconds and to nsteps; without one the sums of the call are dropped, and the call allocates the scratch
 * fields itself ((L + 1) H W float64 words; four more fields of L H W above 40 levels), which the handle then keeps for the
 * next such call until gcm_set_boundary_layer(h, NULL) or gcm_destroy frees them.  On a band that has opted in the call
 * applies the phase to the own rows; like the other explicit calls it requires current ghost rows, and it leaves the
 * ghost rows of u, v, theta and q STALE until the caller's next exchange of the current state (gcm_halo_pack2, the
 * transfer, gcm_halo_unpack2): exchange before anything reads them -- the next stage, gcm_convect_step, gcm_moist_step,
 * gcm_climate_sample.
 * gcm_get_boundary_layer synchronises the handle's stream once; any pointer may be NULL.  gcm_put_boundary_layer uploads
 * sums and counters (restarts): both arrays are required, seconds finite and >= 0, nsteps >= 0.
 * gcm_boundary_layer_reset zeroes all four.
 * Host probes, the routines the kernels call compiled for the host, no handle, no device.  gcm_boundary_layer_surface: the
 * level-0 part of (A) for n columns given uc, vc, theta[0], q[0] and p -> S, z_a, cd [n], any of them may be NULL.
 * gcm_boundary_layer_column: (B) for ncol columns with dsig [L], a [ncol][L-1], x and target [ncol], X [ncol][L] ->
 * X_out [ncol][L] and, where not NULL, X0_surface [ncol] = X0'.
 * Errors, all checked in the call; a refused call changes nothing.  GCM_ERR_ARG: a null handle, no parameters, a
 * non-finite parameter, cd0, cd1, ch or ce < 0, v_cap <= 0, p_strat <= 0, a non-finite dt; the probes: n or ncol < 0,
 * L < 2, a missing array.  GCM_ERR_UNSUPPORTED: other models, L < 2, a sig table that is not strictly decreasing in k
 * (level 0 must be the bottom), a handle created with nranks > 1 that has not opted in
 * (gcm_set_band_boundary_layer).  GCM_ERR_STATE: no ground temperature set
 * (gcm_set_ground) -- reported by gcm_set_boundary_layer itself, not by the next step -- and get, put or reset without a
 * registration.                                                                                                     */
typedef struct {
    double cd0, cd1;             /* drag: cd = cd0 + cd1 S           (7.0e-4, 6.5e-5 s/m)          */
    double v_cap;                /* m/s: cd is held at cd0 + cd1 v_cap for S >= v_cap (20)         */
    double ch, ce;               /* heat and moisture exchange coefficients (0.0044 both)          */
    double p_pbl;                /* Pa: full mixing at and below this pressure (85000)             */
    double p_strat;              /* Pa: e-folding scale of the decay above it (10000)              */
} gcm_boundary_layer;
int gcm_set_boundary_layer(gcm_handle *h, const gcm_boundary_layer *bl);
int gcm_set_band_boundary_layer(gcm_handle *h, int on);
int gcm_band_boundary_layer(const gcm_handle *h);
int gcm_boundary_layer_on(const gcm_handle *h);
int gcm_boundary_layer_step(gcm_handle *h, double dt, const gcm_boundary_layer *bl);
int gcm_get_boundary_layer(gcm_handle *h, double *shf, double *evap, double *seconds, int64_t *nsteps);
int gcm_put_boundary_layer(gcm_handle *h, const double *shf, const double *evap, double seconds, int64_t nsteps);
int gcm_boundary_layer_reset(gcm_handle *h);
int gcm_boundary_layer_surface(int n, const gcm_boundary_layer *bl, double ptop, double sig0, const double *uc,
                               const double *vc, const double *theta0, const double *q0, const double *p,
                               double *S, double *z_a, double *cd);
int gcm_boundary_layer_column(int ncol, int L, const double *dsig, const double *a, const double *x, const double *target,
                              const double *X, double *X_out, double *X0_surface);
/* Slab mixed-layer ocean of GCM_PE25D with a recorded surface and top-of-atmosphere budget, on the device (fp64 and fp32
 * handles; single domains and latitude bands).  Without it the ground temperature is the reference's: a 10 cm slab that
 * the radiation alone heats (gt += dt (B + S - U_s) / Cg / 0.1, in the radiation kernel), and the boundary layer takes
 * sensible heat and water vapour from it for nothing.  With it the ground temperature is the temperature of a slab of heat
 * capacity C (J m^-2 K^-1) that receives the net radiation at the surface, pays for what the boundary layer takes and
 * may receive a prescribed ocean heat flux Q (W / m^2).  Per cell, float64 on either storage type, every operation
 * rounded on its own, in this order (dt the step; S, B, U_s, SH_J, EVAP_KG the flux words below):
 *   R  = (S + B) - U_s       E1 = dt R       E2 = E1 - SH_J       E3 = E2 - Lv EVAP_KG       E4 = E3 + dt Q
 *   gt' = gt + E4 / C
 * C is the scalar heat_capacity (1.0e7: Frierson's 2.4 m of water) or, where given, a field [H][W]; C = +inf holds a cell
 * at its prescribed temperature (E4 / C = 0, and gt + 0 keeps gt's bits).  Q is an optional field [H][W]; none: 0.  The
 * scheme is explicit: it is stable where dt lambda / C << 1, lambda ~ 4 sigma T^3 plus the bulk coefficients' share.
 * Flux words, float64, GCM_SLAB_WORDS fields of [H + 2 ghost rows][W] allocated by the registration and stored by the
 * phases that know them, while the slab is registered and at no other time:
 *   GCM_SLAB_SC       W / m^2   insolation at the top, Sc                       | the radiation kernel's BUDGET
 *   GCM_SLAB_SW_SFC   W / m^2   short wave absorbed by the surface, S           | instantiations, launched in place of the
 *   GCM_SLAB_LW_DOWN  W / m^2   long wave reaching the surface, B               | others by the steps of a registered
 *   GCM_SLAB_LW_UP    W / m^2   long wave leaving the surface, U_s              | handle; they leave gt alone and compute
 *   GCM_SLAB_OLR      W / m^2   up + U_s tcol: up the bottom-up scan's value    | theta exactly as the others do (the
 *                               above the last level, tcol = clw_b_div[L-1] *   | same bits)
 *                               tlw[L-1] formed on the host from the level tables
 *   GCM_SLAB_SH_J     J / m^2   the step's own increment of the boundary layer's shf   | pe_bl_theta_q_kernel, the
 *   GCM_SLAB_EVAP_KG  kg / m^2  the step's own increment of the boundary layer's evap  | same expressions
 * The words of a phase that is not registered count as zero and read as zero.
 * Sums, float64, GCM_SLAB_SUMS fields [H][W] of the own rows, one writer per word and launch, no atomics; the same launch
 * adds  0 dt SC   1 dt S   2 dt B   3 dt U_s   4 dt OLR   5 SH_J   6 Lv EVAP_KG   7 dt Q   8 dt gt'   9 dt gt'^2;
 * seconds (the sum of dt) and nsteps live in the handle.  Time means in W / m^2 are sum / seconds; the surface's net gain
 * is (1 + 2 - 3 - 5 - 6 + 7) / seconds.  The absorbed short wave of the column, ASR = SC - albedo SC csw_top[0], is not
 * summed: albedo and csw_top[0] are constants of the registered physics, so a host forms its sum as
 * sum 0 - albedo / (1 - albedo) sum 1 (albedo < 1), and the top's net gain as ASR - sum 4.
 * gcm_set_slab_ocean(h, so, capacity, qflux): the phase as part of every step taken by gcm_step, gcm_band_run and
 * gcm_end_step: Matsuno step, horizontal diffusion, solar step, Held-Suarez forcing, boundary layer, THIS, convective
 * adjustment, Betts-Miller convection, moist physics, samples.  capacity and qflux are [H][W] or NULL.  It needs
 * gcm_set_ground.  Registering again replaces parameters and fields and resets the sums; so = NULL unregisters and frees
 * everything.  Without a registration nothing is launched or allocated and every result and timing is as before; after
 * an unregistration the radiation advances the ground temperature by the reference's rule again.
 * Latitude bands: the phase is column-local.  A band without the boundary layer advances its ghost rows locally from the
 * neighbour's inputs (their words come from the ghost rows' radiation launch) and adds nothing for them; where a
 * capacity or heat-flux field is registered, which holds own rows only, the ghost rows are left to the next message.  A
 * band with the boundary layer (gcm_set_band_boundary_layer) takes its own rows, in gcm_end_step_begin, ahead of the
 * third exchange, whose message carries the ground temperature's edge rows as every message does: gcm_halo_bytes and the
 * message are unchanged.  Own rows see the single domain's inputs and arithmetic: the same bits, sums included.
 * gcm_slab_ocean_on: 1 where registered, else 0 (other models: 0; a null handle GCM_ERR_ARG).
 * gcm_slab_ocean_apply(h, dt, so, words): uploads words [GCM_SLAB_WORDS][H][W] and applies the cell rule once to the own
 * rows with the parameters so and the registered fields; it adds to the sums, seconds and nsteps only where the slab is
 * registered.  Without a registration the call allocates the words itself, which the handle keeps until
 * gcm_set_slab_ocean(h, NULL, ...) or gcm_destroy.
 * gcm_get_slab_ocean_fluxes(h, words): the words of the last step or apply, own rows, [GCM_SLAB_WORDS][H][W]; one
 * synchronisation.  gcm_get_slab_ocean: sums [GCM_SLAB_SUMS][H][W], seconds, nsteps, any pointer may be NULL;
 * gcm_put_slab_ocean uploads them (restarts): sums required, seconds finite and >= 0, nsteps >= 0; gcm_slab_ocean_reset
 * zeroes all three.
 * gcm_slab_ocean_cells: the cell rule on its own, on the host, the very routine the kernel calls, no handle, no device: n
 * cells with gt [n], words [GCM_SLAB_WORDS][n], C [n] or NULL (the scalar), Q [n] or NULL (0) -> gt_out [n] and, where
 * not NULL, E4_out [n].
 * Errors, all checked in the call; a refused call changes nothing.  GCM_ERR_ARG: a null handle, heat_capacity or a cell of
 * the capacity field NaN or <= 0, Lv not finite or <= 0, a non-finite cell of the heat-flux field, a non-finite dt, a
 * missing array; the probe: n < 0.  GCM_ERR_UNSUPPORTED: other models.  GCM_ERR_STATE: no ground temperature set
 * (gcm_set_ground); fluxes without words in place; get, put or reset without a registration.                        */
enum { GCM_SLAB_SC = 0, GCM_SLAB_SW_SFC = 1, GCM_SLAB_LW_DOWN = 2, GCM_SLAB_LW_UP = 3, GCM_SLAB_OLR = 4, GCM_SLAB_SH_J = 5,
       GCM_SLAB_EVAP_KG = 6, GCM_SLAB_WORDS = 7 };
enum { GCM_SLAB_SUMS = 10 };
typedef struct {
    double heat_capacity;        /* J m^-2 K^-1, > 0; +inf: prescribed temperature (1.0e7)          */
    double Lv;                   /* J / kg: latent heat of vaporisation (2.5e6)                     */
} gcm_slab_ocean;
int gcm_set_slab_ocean(gcm_handle *h, const gcm_slab_ocean *so, const double *capacity, const double *qflux);
int gcm_slab_ocean_on(const gcm_handle *h);
int gcm_slab_ocean_apply(gcm_handle *h, double dt, const gcm_slab_ocean *so, const double *words);
int gcm_get_slab_ocean_fluxes(gcm_handle *h, double *words);
int gcm_get_slab_ocean(gcm_handle *h, double *sums, double *seconds, int64_t *nsteps);
int gcm_put_slab_ocean(gcm_handle *h, const double *sums, double seconds, int64_t nsteps);
int gcm_slab_ocean_reset(gcm_handle *h);
int gcm_slab_ocean_cells(int n, const gcm_slab_ocean *so, double dt, const double *gt, const double *C, const double *words,
                         const double *Q, double *gt_out, double *E4_out);
/* Grey radiation of GCM_PE25D that absorbs by water vapour and CO2, on the device (fp64 and fp32 handles; single domains
 * and latitude bands): the reference's grey_radiation (grey_solar.py:192-320) with clouds off (c = 0), as a phase that
 * takes the solar step's place.  The grey scheme of gcm_set_physics spreads two numbers for the whole planet over the
 * levels; here a level's optical depth comes from its own q and a CO2 mixing ratio, so a moist column and a dry one
 * radiate differently.  Float64 arithmetic on either storage type, every operation rounded on its own, one lane per
 * column.  Per level k (sig, dsig the level table, Rd = 287, G = 9.8, Cp = 1004, sb = 5.67e-8, Cg = 1.13e6):
 *   tp = p sig + ptop     tt = theta exner(tp)     rho = tp / (Rd tt)     depth = (p dsig) / (rho G)
 *   a_sw = 0 + qc rho depth k_h2o_sw + co2 rho depth k_co2_sw      a_lw likewise with the long-wave weights
 *   T_sw = 10^-a_sw       e_lw = 1 - 10^-a_lw      E = sb tt^4 e_lw
 * qc = max(q, 0): a negative q left by the transport cannot give a transmittance above 1; co2 = co2_vmr M_CO2 / Md
 * (44.010 and 28.97 g / mol).  Top-down scan (SWd[L] = SC, LWd[L] = 0): abs_k = SWd (1 - T_sw), SWd -= that;
 * abs_k += LWd e_lw, LWd = LWd - that + E.  Ground (black, albedo a_g): U_s = sb gt^4, gain = (1 - a_g) SWd[0] + LWd[0],
 * dt_ground = (gain - U_s) / Cg / 0.1.  Bottom-up scan (LWu[0] = U_s): abs_k += LWu e_lw, LWu = LWu - that + E.
 * dt_air_k = (abs_k - 2 E) / (Cp rho depth); OLR = LWu[L].  The in-place form is solar_timestep's statements:
 * gt += dt_ground dt, tt += dt_air dt, theta = tt / exner.  The column closes: sum_k Cp rho depth dt_air +
 * (gain - U_s) + a_g SWd[0] + OLR = SC, to rounding.  When both weight pairs are equal (the defaults) the level's power
 * is evaluated once for both bands.
 * Insolation SC: GCM_INSOLATION_UNIFORM, the reference's solar_constant 0.5 0.5; GCM_INSOLATION_ZENITH, solar_constant
 * max(sin lat sin d + cos lat cos d cos(lon + hour_angle), 0) with the hour angle of the grey kernel
 * (utc / (-24 h) 360 degrees) and the fixed declination d; GCM_INSOLATION_DAILY, the reference's
 * daily_average_irradiance(lat, d) with solar_constant, a host-built table per global row, the arccos argument kept
 * inside [-1, 1] (the reference gives NaN in polar night and polar day: the one departure from it).
 * gcm_set_gas_radiation(h, par): while gcm_set_physics is on AND this is registered, the solar step of every step taken
 * by gcm_step, gcm_band_run and gcm_end_step launches this kernel instead of the grey one, at the physics registration's
 * clock, lat and lon; its t_lw, t_sw and albedo are then unused.  Registering without physics is allowed and takes
 * effect when physics comes on.  It needs gcm_set_ground.  par = NULL unregisters: the grey scheme again.  Without a
 * registration nothing is launched, allocated or changed on any path.  While the slab ocean is registered the launch
 * leaves the ground temperature to it and stores the flux words GCM_SLAB_SC = SC, GCM_SLAB_SW_SFC = (1 - a_g) SWd[0],
 * GCM_SLAB_LW_DOWN = LWd[0], GCM_SLAB_LW_UP = U_s and GCM_SLAB_OLR = LWu[L]; the short wave the surface sends back to
 * space is then a_g SW_SFC / (1 - a_g).  Latitude bands: the phase is column-local, q travels in the message already;
 * ghost rows are advanced locally with the latitude of their global row, to the neighbour's bits.
 * gcm_gas_radiation_on: 1 where registered, else 0 (a null handle GCM_ERR_ARG).
 * gcm_gas_radiation(h, utc, par, lat, lon, dt_ground, dt_air, olr): the diagnostic form on the current state: lat
 * [global_height], lon [W]; dt_ground [H][W], dt_air [L][H][W], olr [H][W], any of them may be NULL; dt_air passes
 * through the handle's storage type, dt_ground and olr are float64.  gcm_gas_radiation_step(h, dt, utc, par, lat, lon):
 * once in place; on a band own rows and ghost rows, as gcm_solar_step.
 * gcm_gas_radiation_columns: the column routine on its own, on the host, the very routine the kernel calls, no handle, no
 * device: ncol columns with SC, p, gt [ncol], the true temperature tt and q [L][ncol], sig and dsig [L] -> dt_ground
 * [ncol], dt_air [L][ncol], olr [ncol] and words [5][ncol] in the order GCM_SLAB_SC .. GCM_SLAB_OLR; any output may be NULL.
 * gcm_gas_insolation(kind, nlat, lat, declination, solar_constant, out): the row table out [nlat] of "uniform" and
 * "daily"; "zenith" has none (GCM_ERR_ARG).
 * Errors, all checked in the call; a refused call changes nothing.  GCM_ERR_ARG: a null handle, a weight, co2_vmr or
 * solar_constant that is not finite or negative, ground_albedo outside [0, 1), |declination| > pi / 2, an unknown
 * insolation, a non-finite utc or dt, missing lat or lon.  GCM_ERR_UNSUPPORTED: other models, more than 120 levels.
 * GCM_ERR_STATE: no ground temperature set (gcm_set_ground).                                                             */
enum { GCM_INSOLATION_UNIFORM = 0, GCM_INSOLATION_ZENITH = 1, GCM_INSOLATION_DAILY = 2 };
typedef struct {
    double k_h2o_lw;             /* m^2 / kg: long-wave weight of water vapour (0.125)                */
    double k_co2_lw;             /* m^2 / kg: long-wave weight of CO2 (1)                             */
    double k_h2o_sw;             /* m^2 / kg: short-wave weight of water vapour (0.125)               */
    double k_co2_sw;             /* m^2 / kg: short-wave weight of CO2 (1: the reference's placeholder) */
    double co2_vmr;              /* volume mixing ratio of CO2 (300e-6)                               */
    double ground_albedo;        /* [0, 1) (0.1)                                                      */
    double solar_constant;       /* W / m^2 (2 * 41840 / 60)                                          */
    double declination;          /* radians, |d| <= pi / 2 (0)                                        */
    int32_t insolation;          /* GCM_INSOLATION_* (GCM_INSOLATION_UNIFORM)                         */
} gcm_gas_radiation_par;
int gcm_set_gas_radiation(gcm_handle *h, const gcm_gas_radiation_par *par);
int gcm_gas_radiation_on(const gcm_handle *h);
int gcm_gas_radiation(gcm_handle *h, double utc, const gcm_gas_radiation_par *par, const double *lat, const double *lon,
                      double *dt_ground, double *dt_air, double *olr);
int gcm_gas_radiation_step(gcm_handle *h, double dt, double utc, const gcm_gas_radiation_par *par, const double *lat, const double *lon);
int gcm_gas_radiation_columns(int ncol, int L, const gcm_gas_radiation_par *par, const double *SC, const double *p, double ptop,
                              const double *sig, const double *dsig, const double *tt, const double *q, const double *gt,
                              double *dt_ground, double *dt_air, double *olr, double *words);
int gcm_gas_insolation(int kind, int nlat, const double *lat, double declination, double solar_constant, double *out);
/* Zonal-mean climatology of GCM_PE25D accumulated on the device: what a Held-Suarez run is evaluated by -- the time and
 * zonal means of u, v, theta and T, their variances and the eddy fluxes as functions of latitude and level -- without a
 * host round trip per step (fp64 and fp32 handles, single domains and latitude bands).  One launch per sample reads
 * the current state once and adds, per own row j and level k, the zonal sums over i = 0 .. W - 1 of the moments below
 * to float64 sums that live in the handle; plain sums, not divided by W: the host divides by W nsamples.
 * Values are widened exactly from the storage type; every product and sum is float64 and rounded on its own.
 *   m3 [GCM_CLIM_WORDS3][L][H]:  0 u   1 v   2 theta   3 T = theta Pi   4 u u   5 v v   6 T T
 *                                7 uc vc   8 vc T   9 vc theta          (u, v at their own C-grid points)
 *   m2 [GCM_CLIM_WORDS2][H]:     0 p   1 p p
 *   Pi = (p_lev / P0)^kappa, p_lev = sig[k] p + ptop, from the kernels' own Exner routine (the one the Held-Suarez
 *   and radiation kernels use: within the 1e-10 of the parity tests of pow);
 *   uc = 0.5 (u[i] + u[i - 1]), periodic in i;  vc = 0.5 (v[j] + v[j - 1]): the winds at the cell centre.
 *   Row -1 of a single domain is row H - 1, the model's own pole-to-pole roll, reproduced and not fixed; on a band it
 *   is the first north ghost row of v of the current state.
 * Reduction order of a row's W terms -- a function of W alone, whatever H, the band, the number of CUs or the number of
 * levels a workgroup walks: 256 partial sums, partial sum t takes i = t, t + 256, ... in that order, starting from
 * 0.0; they are 4 groups of 64 (t / 64); within a group the 64 combine by the butterfly x[t] <- x[t] + x[t ^ d],
 * d = 32, 16, 8, 4, 2, 1; the four groups' results are added in group order; the row's sum is then added to the
 * accumulator word, sample after sample.  One writer per word and launch, no atomics: the same state gives the same
 * bits, and a band's rows hold the bits of the same rows of the single domain.
 * gcm_set_climate(every >= 1) allocates and zeroes the sums and the sample count and starts a step counter at 0; from
 * then on every step taken by gcm_step and gcm_band_run ends -- behind the solar step and the Held-Suarez forcing --
 * with a sample where the counter, incremented per step, is a multiple of `every`.  The counter runs across calls.
 * gcm_half_step (and a band stepped by gcm_step_phase) never samples.  Registering again resets the sums; every = 0
 * unregisters and frees; every < 0: GCM_ERR_ARG.  Without a registration nothing is launched and every result and
 * timing is as before; a sample changes nothing a step reads.
 * gcm_climate_every: the registered `every`, 0 without one (other models: 0; a null handle GCM_ERR_ARG).
 * gcm_climate_sample: one sample now; the step counter is untouched.  On a band the ghost rows of the current state
 * must be current, as for gcm_solar_step and gcm_held_suarez_step.
 * gcm_climate_reset zeroes the sums and the count.  gcm_get_climate synchronises the handle's stream once and copies
 * the sums and the count; any of the three pointers may be NULL.  gcm_put_climate uploads them (restarts); both
 * arrays are required, nsamples >= 0.
 * Errors: a null handle GCM_ERR_ARG; other models GCM_ERR_UNSUPPORTED (and a row too wide for the sample's LDS, more
 * than ~7800 columns); get, put, reset or sample without a registration GCM_ERR_STATE.  A refused call changes nothing. */
#define GCM_CLIM_WORDS3 10   /* moments per (level, row) */
#define GCM_CLIM_WORDS2 2    /* moments per row          */
int gcm_set_climate(gcm_handle *h, int every);
int gcm_climate_every(const gcm_handle *h);
int gcm_climate_sample(gcm_handle *h);
int gcm_climate_reset(gcm_handle *h);
int gcm_get_climate(gcm_handle *h, double *m3, double *m2, int64_t *nsamples);
int gcm_put_climate(gcm_handle *h, const double *m3, const double *m2, int64_t nsamples);
/* GCM_PE25D on pressure levels: the sigma -> p step on the device.  The climatology and the spectra above live on the
 * model's sigma surfaces; figures are drawn against pressure, and over topography a zonal mean along sigma mixes air of
 * very different pressures.  Every column of the current state is interpolated to a fixed list of pressures and masked
 * where the pressure lies under the ground or above the top mid-level; the result comes back as maps (gcm_plev_fields)
 * or is reduced zonally into float64 sums that live in the handle (gcm_set_plev_climate), the way the sigma climatology
 * is.  fp64 and fp32 handles, single domains and latitude bands.
 * The column rule -- float64, storage values widened exactly, every operation rounded on its own (no contraction):
 *   Levels run k = 0 (bottom) .. L - 1 (top), as the geometry has them.  pl[k] = sig[k] p + ptop, p the handle's p
 *   field (surface pressure minus ptop); pl decreases strictly with k wherever p > 0.
 *   Targets P[n], n = 0 .. N - 1, in Pa: full pressure, finite, positive and strictly decreasing (the direction of k),
 *   1 <= N <= GCM_PLEV_MAX.
 *   Target n of a column is VALID iff pl[L - 1] <= P[n] <= pl[0] (and pl[L - 1] < pl[0]): no extrapolation, below the
 *   ground or above the top mid-level.  A column with p <= 0 or a NaN p has no valid target.
 *   For a valid target: k is the largest index in 0 .. L - 2 with pl[k] >= P[n];  w = (pl[k] - P[n]) / (pl[k] - pl[k + 1])
 *   (the correctly rounded float64 division);  x_n = (1 - w) x[k] + w x[k + 1]: a target that sits exactly on a level
 *   returns that level's value exactly.  NaN in a value propagates; it never decides validity.
 *   Linear in pressure on purpose: the rule needs no transcendental, so the mask and the interpolated uc, vc, theta and q
 *   can be restated bit for bit.  Log-pressure weights are not offered; the geopotential height on the same targets,
 *   which is not linear in p, has calls of its own (gcm_plev_height, gcm_set_plev_maps below).
 * Five cell-centre quantities are interpolated, formed per level exactly as the climatology forms them:
 *   uc = 0.5 (u[i] + u[i - 1]), periodic in i;  vc = 0.5 (v[j] + v[j - 1]);  theta;  T = theta Pi(pl), formed on the
 *   sigma level with the kernels' own Exner routine and then interpolated;  q.  Row -1 is row H - 1 on a single domain
 *   and v's first north ghost row on a band.
 * gcm_plev_columns: the host build of the rule, from the header the kernels compile from; no handle, no device.  pl and
 *   x are [ncol][L], out and valid [ncol][N]; out is left untouched where a target is invalid.  GCM_ERR_ARG: a null
 *   pointer, L < 2, N out of range, targets that are not strictly decreasing, positive and finite.
 * gcm_plev_fields: one launch interpolates the current state's five quantities to the N targets.  out [5][N][H][W]
 *   float64 in the order uc, vc, theta, T, q; an invalid entry holds `fill`.  valid [N][H][W] may be NULL.  The call
 *   holds 8 * 5 * N * H * W bytes of device memory for its duration (4 N H W more where valid is asked for) and releases
 *   them: it is meant for a handful of levels now and then, not for all of them every step.  On a band the ghost rows
 *   must be current, as for gcm_climate_sample.  A pure reader of the state; it synchronises the handle's stream.
 * gcm_set_plev_climate(every >= 1, N, P): the accumulating sample.  Sums s [GCM_PLEV_WORDS][N][H], float64, plain sums
 *   over i and over the samples; nothing is divided on the device:
 *     0 count (1.0 per valid column)   1 uc   2 vc   3 theta   4 T   5 q   6 uc uc   7 vc vc   8 T T   9 uc vc
 *     10 vc T   11 vc theta   12 vc q            (products of the interpolated values)
 *   An invalid column contributes 0.0 to every word; the host forms the conditional means s[w] / s[0].
 *   Reduction order of a row's W terms: the climatology's, a function of W alone -- 256 partial sums over
 *   i = t, t + 256, ... starting from 0.0, the butterfly x[t] <- x[t] + x[t ^ d], d = 32 .. 1, within each 64, the four
 *   groups in order; the row's sum is then added to the accumulator word, sample after sample.  One writer per word and
 *   launch, no atomics.  A row's contribution does not depend on H, the band, the CU count or how the targets are split
 *   over the grid: a band's rows hold the bits of the same rows of the single domain.
 *   The registration allocates and zeroes the sums, copies the targets and starts a step counter of its own; it holds
 *   8 (N + GCM_PLEV_WORDS N H) bytes on the device.  From then on every `every`-th step of gcm_step, gcm_band_run and
 *   gcm_end_step / gcm_end_step_finish ends with one sample, directly behind the sigma climatology's and ahead of the
 *   spectra's; on a band the compute stream joins the exchange stream's tail once for all the samples due on that step.
 *   gcm_half_step and gcm_step_phase never sample.  Registering again resets sums, count and counter; every = 0
 *   unregisters and frees.  Without a registration nothing is launched and every result and timing is as before; a
 *   sample changes nothing a step reads.
 * gcm_plev_climate_every: the registered `every`, 0 without one (other models: 0).  gcm_plev_climate_levels: copies up
 *   to cap targets to P (may be NULL) and returns N.  gcm_plev_climate_sample: one sample now, the counter untouched; a
 *   band's ghost rows must be current.  gcm_plev_climate_reset zeroes the sums and the count.  gcm_get_plev_climate
 *   synchronises the handle's stream once and copies the sums and the count; either pointer may be NULL.
 *   gcm_put_plev_climate uploads them (restarts): s is required, nsamples >= 0.
 * gcm_plev_climate_plan: the launch geometry of a sample, without launching, GCM_PLEV_PLAN_WORDS words:
 *   [0] grid x = rows  [1] target segments (grid y; 0 without a registration)  [2] targets per segment  [3] threads
 *   [4] LDS bytes  [5] 256-column chunks per row.  A segment reads, per column, only the levels that bracket its targets.
 * Errors, all checked in the call; a refused call changes nothing.  GCM_ERR_ARG: a null handle, every < 0, bad targets.
 * GCM_ERR_UNSUPPORTED: other models, L < 2.  (A thread keeps its column's p in a register, so no row is too wide for the
 * launch's LDS.)  GCM_ERR_STATE: levels, get, put, reset or sample without a registration.  GCM_ERR_HIP: an allocation
 * that fails; nothing stays registered then.                                                                          */
#define GCM_PLEV_MAX 64         /* targets of a call or a registration */
#define GCM_PLEV_WORDS 13       /* sums per (target, row)              */
#define GCM_PLEV_PLAN_WORDS 6
int gcm_plev_columns(int ncol, int L, int N, const double *pl, const double *x, const double *P, double *out, int *valid);
int gcm_plev_fields(gcm_handle *h, int N, const double *P, double fill, double *out, int32_t *valid);
int gcm_set_plev_climate(gcm_handle *h, int every, int N, const double *P);
int gcm_plev_climate_every(const gcm_handle *h);
int gcm_plev_climate_levels(const gcm_handle *h, double *P, int cap);
int gcm_plev_climate_sample(gcm_handle *h);
int gcm_plev_climate_reset(gcm_handle *h);
int gcm_get_plev_climate(gcm_handle *h, double *s, int64_t *nsamples);
int gcm_put_plev_climate(gcm_handle *h, const double *s, int64_t nsamples);
int gcm_plev_climate_plan(gcm_handle *h, int *out, int nout);
/* GCM_PE25D: geopotential height on pressure levels, and time-mean maps that keep longitude.  Z500 is the first map
 * drawn of such a run -- its variance is the storm track, its time mean over topography (gcm_config.heightmap) the
 * stationary waves -- and the three accumulators above all collapse longitude.  fp64 and fp32 handles, single domains
 * and latitude bands.
 * The column rule -- float64, storage values widened exactly, every operation rounded on its own (no contraction), the
 * divisions correctly rounded; levels, targets P[n], validity and bracket exactly as for the pressure levels above:
 *   The mid-level geopotential is the model's, in its summation order, Pi = (pl / P0)^kappa by the kernels' own Exner
 *   routine:   rho[k] = pl[k] / (Rd (theta[k] Pi[k]));   s1[k] = ((sig[k] p) / rho[k]) dsig[k];
 *   stp[k] = (Cp (0.5 (theta[k] + theta[k + 1]))) (Pi[k] - Pi[k + 1]), k + 1 = L taken as 0, as the model has it;
 *   s2[k] = sigt[k] stp[k];   phi[0] = (sum_k (s1[k] - s2[k]), k ascending from 0.0) + heightmap G, the heightmap's row
 *   being the global row (row0 + j on a band);   phi[k] = phi[k - 1] + stp[k - 1].
 *   (The model's step takes a reciprocal approximation for 1 / rho: its phi agrees with this one to rounding, not bit
 *   for bit.)
 *   For a valid target in bracket k the height continues the model's hydrostatic relation inside the layer, linear in Pi
 *   and not in p:   Z[n] = (phi[k] + (Cp (0.5 (theta[k] + theta[k + 1]))) (Pi(pl[k]) - Pi(P[n]))) / G.
 *   A target that sits exactly on a level returns that level's phi / G exactly, whichever of its two brackets it is
 *   evaluated in.  No extrapolation under the ground or above the top mid-level.  NaN in theta propagates and never
 *   decides validity; a column with p <= 0 or a NaN p has no valid target.
 * gcm_plev_height_columns: the host build of the rule, from the header the kernel compiles from; no handle, no device.
 *   p [ncol], theta [ncol][L], hmG [ncol] (heightmap G per column; NULL: 0), sig, dsig, sigt [L], out and valid
 *   [ncol][N]; out is left untouched where a target is invalid.  GCM_ERR_ARG: a null pointer other than hmG, ncol < 0,
 *   L < 2, a ptop that is not finite, N out of range, targets that are not strictly decreasing, positive and finite.
 * gcm_plev_height: one launch over the current state.  out [N][H][W] float64 in metres; an invalid entry holds `fill`.
 *   valid [N][H][W] may be NULL.  The call holds 8 N H W bytes of device memory for its duration (4 N H W more where
 *   valid is asked for) and releases them.  On a band the ghost rows need not be current: the height reads theta and p
 *   of own rows only.  A pure reader of the state; it synchronises the handle's stream.
 * gcm_set_plev_maps(every >= 1, N, P): the accumulating sample.  Sums s [GCM_PLEV_MAP_WORDS][N][H][W], float64, plain sums
 *   over the samples; nothing is divided or reduced along i on the device:
 *     0 count (1.0 per valid sample)   1 Z   2 Z Z   3 T   4 T T   5 uc   6 vc   7 uc uc   8 vc vc   9 uc vc   10 vc T
 *     11 q   12 vc q
 *   T = theta Pi, uc, vc and q are the pressure-level quantities above, interpolated linearly in p by the same routines:
 *   the bits gcm_plev_fields returns; Z the bits gcm_plev_height returns; the products are products of those.  A sample
 *   in which the target is invalid in a column adds nothing to that column's words: the host forms the conditional
 *   means s[w] / s[0].  And s2 [GCM_PLEV_MAP_WORDS2][H][W]: p and p p of every column and sample.
 *   One writer per accumulator word and launch, no atomics, no reduction across columns: a cell's sums depend on that
 *   column's data only -- not on H, W, the band or the CU count -- and a band's rows hold the bits of the same rows of
 *   the single domain.
 *   The registration allocates and zeroes the sums, copies the targets and starts a step counter of its own; it holds
 *   8 (N + (GCM_PLEV_MAP_WORDS N + GCM_PLEV_MAP_WORDS2) H W) bytes on the device -- 340 MB at 1440 x 720 with three
 *   targets: it is meant for a handful of levels, not for all of them -- besides a level table of 24 L bytes that the
 *   handle keeps.  From then on every `every`-th step of gcm_step, gcm_band_run and gcm_end_step / gcm_end_step_finish
 *   ends with one sample, behind the spectra's; on a band the compute stream joins the exchange stream's tail once for
 *   all the samples due on that step.  gcm_half_step and gcm_step_phase never sample.  Registering again resets sums,
 *   count and counter; every = 0 unregisters and frees.  Without a registration nothing is launched and every result
 *   and timing is as before; a sample changes nothing a step reads.
 * gcm_plev_maps_every: the registered `every`, 0 without one (other models: 0).  gcm_plev_maps_levels: copies up to cap
 *   targets to P (may be NULL) and returns N.  gcm_plev_maps_sample: one sample now, the counter untouched; a band's
 *   ghost rows must be current (vc reads v's first north ghost row).  gcm_plev_maps_reset zeroes the sums and the count.
 *   gcm_get_plev_maps synchronises the handle's stream once and copies the sums and the count; any of the three pointers
 *   may be NULL.  gcm_put_plev_maps uploads them (restarts): s and s2 are required, nsamples >= 0.
 * gcm_plev_maps_plan: the launch geometry of a sample, without launching, GCM_PLEV_MAP_PLAN_WORDS words:
 *   [0] grid x = 256-column chunks of a row  [1] grid y = rows (0 without a registration: no work)  [2] threads
 *   [3] LDS bytes  [4] targets (0 without a registration).  One kernel path serves every L: a lane reads its theta
 *   column twice, the second time from cache.
 * Errors, all checked in the call; a refused call changes nothing.  GCM_ERR_ARG: a null handle, every < 0, bad targets, a
 * null out.  GCM_ERR_UNSUPPORTED: other models, L < 2.  GCM_ERR_STATE: levels, get, put, reset or sample without a
 * registration.  GCM_ERR_HIP: an allocation that fails; nothing stays registered then.                              */
#define GCM_PLEV_MAP_WORDS 13      /* sums per (target, cell) */
#define GCM_PLEV_MAP_WORDS2 2      /* sums per cell           */
#define GCM_PLEV_MAP_PLAN_WORDS 5
int gcm_plev_height_columns(int ncol, int L, int N, const double *p, const double *theta, const double *hmG, const double *sig,
                            const double *dsig, const double *sigt, double ptop, const double *P, double *out, int *valid);
int gcm_plev_height(gcm_handle *h, int N, const double *P, double fill, double *out, int32_t *valid);
int gcm_set_plev_maps(gcm_handle *h, int every, int N, const double *P);
int gcm_plev_maps_every(const gcm_handle *h);
int gcm_plev_maps_levels(const gcm_handle *h, double *P, int cap);
int gcm_plev_maps_sample(gcm_handle *h);
int gcm_plev_maps_reset(gcm_handle *h);
int gcm_get_plev_maps(gcm_handle *h, double *s, double *s2, int64_t *nsamples);
int gcm_put_plev_maps(gcm_handle *h, const double *s, const double *s2, int64_t nsamples);
int gcm_plev_maps_plan(gcm_handle *h, int *out, int nout);
/* Zonal wavenumber spectra of GCM_PE25D accumulated on the device: the kinetic-energy and temperature spectra by zonal
 * wavenumber and the split of the eddy momentum and heat fluxes over the waves, which the zonal sums of the climatology
 * cannot give, without a host round trip per step (fp64 and fp32 handles, single domains and latitude bands).  One launch
 * per sample reads the current state once.  For every own row j and level k it forms four real rows of length W in
 * float64 -- storage values widened exactly, every product and sum float64 and rounded on its own (no contraction):
 *   uc = 0.5 (u[i] + u[i - 1]), periodic in i;   vc = 0.5 (v[j] + v[j - 1]);   theta;   T = theta Pi(sig[k] p + ptop)
 *   Row -1 is the climatology's: row H - 1 on a single domain, the first north ghost row of v on a band.  Pi comes from
 *   the kernels' own Exner routine (within the 1e-10 of the parity tests of pow).
 * Their discrete Fourier transforms along i, X_m = sum_i x_i exp(-2 pi i m i / W) (NumPy's convention), are taken in
 * float64 on every handle, with a float64 twiddle table of the registration's own (W entries, built on the host from
 * angles reduced to an octant in integers).  For m = 0 .. mmax the launch adds the raw products to float64 sums
 *   s [GCM_SPEC_WORDS][L][H][M],  M = mmax + 1, m the fastest index:
 *   0 uu = |Uc|^2   1 vv = |Vc|^2   2 TT = |That|^2   3 uv = Re(Uc conj Vc)   4 vT = Re(Vc conj That)
 *   5 vtheta = Re(Vc conj Thetahat)
 * Plain sums over the samples; nothing is divided on the device.  Words 3 - 5 are the wavenumber split of the
 * climatology's words 7 - 9, word 2 that of its word 6: with mmax = W / 2 and the one-sided weights w_m = 1 for m = 0 and
 * m = W / 2 (even W), w_m = 2 otherwise, sum_m w_m s[word][m] / W is the corresponding zonal sum up to rounding.  The
 * one-sided spectrum per sample is w_m s / (W W nsamples): a row's entries then sum to the zonal mean of the product.
 * How it is computed: per level two complex transforms in LDS, z1 = uc + i vc and z2 = T + i theta (the mixed-radix
 * Stockham passes of the polar filter's generic path, the radices of W in the order 4s, 2s, odd primes
 * ascending); the packed rows come apart as X_m = (Z_m + conj Z_{W-m}) / 2, Y_m = (Z_m - conj Z_{W-m}) / (2i), index
 * W - m at m = 0 taken as 0.  A product is Re(A conj B) = A.re B.re + A.im B.im.
 * Determinism: each accumulator word has one writer per launch, no atomics.  What a row contributes depends on that
 * row's data, W and mmax only -- not on H, the band, the CU count or how levels are split over the grid; the transform's
 * path is chosen from W alone.  The same state gives the same bits, and a band's rows hold the bits of the same rows of
 * the single domain.
 * gcm_set_spectra(every >= 1, mmax) allocates and zeroes the sums and the sample count and starts a step counter of the
 * spectra's own at 0; mmax = -1: min(W / 2, 63).  From then on every step taken by gcm_step, gcm_band_run and
 * gcm_end_step / gcm_end_step_finish ends -- directly behind the climatology's sample where that is due -- with a
 * sample where the counter, incremented per step, is a multiple of `every`.  The counter runs across calls.  On a band
 * the compute stream joins the exchange stream's tail before the sample, once for both diagnostics.  gcm_half_step and
 * gcm_step_phase never sample.  Registering again resets the sums and the counters; every = 0 unregisters and frees.
 * Without a registration nothing is launched and every result and timing is as before; a sample changes nothing a step
 * reads.  A registration holds 8 (2 W + L + GCM_SPEC_WORDS L H M) bytes on the device: 53.1 MB at 1440 x 720 x 24 with
 * the default mmax.  The launch takes 32 W + 8 W + 2048 bytes of LDS (W odd: 8 more).
 * gcm_spectra_every: the registered `every`, 0 without one (other models: 0; a null handle GCM_ERR_ARG).
 * gcm_spectra_mmax: the registered mmax; GCM_ERR_STATE without a registration.
 * gcm_spectra_sample: one sample now; the step counter is untouched.  On a band the ghost rows of the current state
 * must be current.  gcm_spectra_reset zeroes the sums and the count.  gcm_get_spectra synchronises the handle's stream
 * once and copies the sums and the count; either pointer may be NULL.  gcm_put_spectra uploads them (restarts): s is
 * required, nsamples >= 0.
 * gcm_spectra_plan: the launch geometry of a sample of this handle, without launching, GCM_SPEC_PLAN_WORDS words:
 *   [0] grid x = rows  [1] level segments (grid y)  [2] threads  [3] LDS bytes  [4] passes of a transform
 *   [5] wavenumbers a thread holds (at the registered mmax, else at the default)
 * Errors, all checked in the call; a refused call changes nothing.  GCM_ERR_ARG: a null handle, every < 0, mmax < -1 or
 * mmax > W / 2.  GCM_ERR_UNSUPPORTED: other models, and a row whose transform buffers do not fit the 160 KB of LDS a
 * launch may ask for (W > 4044; the message states the width).  GCM_ERR_STATE: get, put, reset, sample or mmax without
 * a registration.  GCM_ERR_HIP: an allocation that fails; nothing stays registered then.                          */
#define GCM_SPEC_WORDS 6        /* products per (level, row, wavenumber) */
#define GCM_SPEC_PLAN_WORDS 6
int gcm_set_spectra(gcm_handle *h, int every, int mmax);
int gcm_spectra_every(const gcm_handle *h);
int gcm_spectra_mmax(const gcm_handle *h);
int gcm_spectra_plan(gcm_handle *h, int *out, int nout);
int gcm_spectra_sample(gcm_handle *h);
int gcm_spectra_reset(gcm_handle *h);
int gcm_get_spectra(gcm_handle *h, double *s, int64_t *nsamples);
int gcm_put_spectra(gcm_handle *h, const double *s, int64_t nsamples);
/* Horizontal del-2 / del-4 diffusion of u, v, theta (and q) of GCM_PE25D on the device: the scale-selective dissipation a
 * lat-lon C-grid run needs besides the polar filter, which acts along i at high latitudes only (fp64 and fp32 handles;
 * single domains, and latitude bands that have opted in: gcm_set_band_hdiff).  gcm_set_hdiff registers it as a phase of every step taken by gcm_step, applied once per step
 * directly behind the Matsuno step and ahead of the solar step; gcm_half_step and gcm_step_phase never apply it.
 * Grid: centres are (j, i); u lies between centres i and i + 1 on the centre latitude of row j; v lies between rows j
 * and j + 1, on dx_h[j]'s latitude.  i and j are periodic, as in the dynamics.  The diffusion acts on the model's sigma
 * surfaces, level by level, and component-wise on u and v: no metric terms of the vector Laplacian.
 * Host tables, float64, every operation rounded on its own, from the handle's own dx_j, dx_h, dy over the global height
 * (gcm_hdiff_tables builds the same ones without a handle or a device; out is [8][H]: ax bn bs area axv bnv bsv areav):
 *   s = nu dt (order 1, nu in m^2/s);   s = sqrt(nu dt) (order 2, nu in m^4/s);   ay = min(s / (dy dy), cmax)
 *   centre rows (theta, q, u):
 *     ax[j] = min(s / (dx_j[j] dx_j[j]), cmax);   area[j] = ((dx_h[j-1] + dx_h[j]) dy) 0.5
 *     bs[j] = (ay (dx_h[j] dy)) / area[j];        bn[j] = (ay (dx_h[j-1] dy)) / area[j]
 *   v rows:
 *     axv[j] = min(s / (dx_h[j] dx_h[j]), cmax);  areav[j] = ((dx_j[j] + dx_j[j+1]) dy) 0.5
 *     bsv[j] = (ay (dx_j[j+1] dy)) / areav[j];    bnv[j] = (ay (dx_j[j] dy)) / areav[j]
 * The min is what keeps the explicit step stable where the meridians converge: rows near the poles run at the capped
 * diffusion number, the others at the physical coefficient; a division by a tiny dx_h at the pole row gives a large or
 * infinite quotient, which the min caps.
 * Update, float64 arithmetic for either storage type, no contraction, the result rounded once to the storage type:
 *   zx = (X[j][i+1] - X[j][i]) - (X[j][i] - X[j][i-1]);   gs = X[j+1][i] - X[j][i];   gn = X[j][i] - X[j-1][i]
 *   D(X) = ax[j] zx + (bs[j] gs - bn[j] gn)                                  (v: axv, bsv, bnv)
 *   order 1: X' = X + D(X);   order 2: Y = D(X) kept in float64, never rounded to storage; X' = X - D(Y)
 * Every operation is an IEEE add, subtract or multiply with host-built coefficients: the device result equals a NumPy
 * restatement bit for bit in both storage types, whichever tile computes a cell.  With 0 < cmax <= 1/8,
 * 4 ax + 2 (bn + bs) <= 1: order 1 obeys the maximum principle per level, order 2 has an amplification factor in
 * [0, 1] for every mode, and sum_j area[j] sum_i X per level is conserved up to rounding (the meridional fluxes telescope).
 * fields is a mask of GCM_HDIFF_U, _V, _T, _Q.  Unselected fields, p, the passive tracers and the ground temperature are
 * neither read nor written.  The launch is out of place: it writes landing fields of the handle's real type ([H][L][W]
 * per selected field, allocated by the registration or by the first explicit step and kept until gcm_set_hdiff(h, NULL)
 * or gcm_destroy), which the state then takes over by a device copy on the same stream.
 * Limits: latitude bands (nranks > 1) are refused by default -- the phase is not column-local, at order 2 it reads two
 * rows beyond the own rows, and a band's ghost rows cannot be advanced locally: a band needs an exchange of its own
 * behind the phase, which the opt-in below buys; p and the passive tracers are not diffused; theta is not pressure-weighted (the diffusion
 * conserves sum area theta per level, not the mass-weighted sum); over topography it mixes along sigma surfaces, not
 * pressure surfaces; no vector-Laplacian metric terms; the cap stands in for an implicit zonal solve.
 * gcm_set_hdiff(h, d) registers (d == NULL: off, and frees the landing fields and tables); registering again replaces the
 * parameters.  Without a registration nothing is launched and every result and timing is as before.  The device tables
 * are rebuilt when a step comes with another dt, not on every step.
 * gcm_hdiff_on: 1 where the phase is registered, else 0 (other models: 0; a null handle GCM_ERR_ARG).
 * gcm_hdiff_step: the same launch once, in place on the current state, with d's parameters and no registration.
 * gcm_hdiff_apply: the host build of the very cell routine the kernel calls, over X [nlev][H][W] float64 with tab4 [4][H]
 * = ax bn bs area (or the v rows' four), periodic both ways, into out; no handle, no device.
 * Latitude bands.  gcm_set_band_hdiff(h, on): GCM_PE25D latitude bands only -- other models, and a single domain with
 * on != 0, are GCM_ERR_UNSUPPORTED (on = 0 on a single domain: nothing to do); called right after gcm_create, on every
 * band of a run; on = 0 while the phase is registered is GCM_ERR_STATE; a null handle GCM_ERR_ARG; a refused call changes
 * nothing.  The opt-in alone launches nothing and changes no result, message size (gcm_halo_bytes) or timing; without it
 * a band stays refused.  gcm_band_hdiff: 1 on a band that has opted in, else 0 (a null handle GCM_ERR_ARG).  After the
 * opt-in gcm_set_hdiff and gcm_hdiff_step are accepted (W >= 4, 2 own rows or more).  A band's u, v, theta and q carry
 * two ghost rows a side, the phase sits directly behind the corrector, whose exchange has just filled them, and the
 * order-2 stencil has radius 2: the band's own rows are diffused from what is there, with the coefficients of the
 * global rows (row0 + j) mod global_height, to the single domain's bits.  The ghost rows themselves cannot be (ghost
 * row -1 would need row -3): they are stale behind the launch, and the current state's edge rows are exchanged once
 * more before anything reads them -- one more message of gcm_halo_bytes per neighbour and step, in the existing message
 * and buffers.  With the phase registered gcm_band_run does that itself under every orchestration: the own rows'
 * diffusion and its copy back behind the corrector's unpack, the pack, the exchange, the unpack, then the ghost rows'
 * phases and the walk as without it (with the boundary layer registered too: four exchanges per step).  A host that
 * drives the exchange itself: gcm_end_step_diffuse below.  gcm_hdiff_step on a band diffuses the own rows from current
 * ghost rows and leaves the ghost rows of the selected fields stale until the caller's next exchange.
 * gcm_hdiff_apply_band: the host build of the band walk, periodic in i only: X [nlev][Hb + 4][W] float64 holds the
 * band's Hb own rows with two ghost rows a side (rows -2 .. Hb + 1), tab4 [4][Hb + 4] = ax bn bs area (or the v rows'
 * four) of those rows, out [nlev][Hb][W] the own rows -- rows [row0, row0 + Hb) of gcm_hdiff_apply over the periodic
 * whole, bit for bit; no handle, no device.
 * gcm_hdiff_plan: the launch geometry of this handle without launching (a band: its own rows' tiles), GCM_HDIFF_PLAN_WORDS words, at the registered
 * order and fields, else at order 2 and U|V|T:
 *   [0] tile rows  [1] tile columns  [2] tiles in i  [3] tiles in j  [4] grid z (selected fields x levels)
 *   [5] LDS bytes  [6] kernel launches per application
 * Errors, all checked in the call; a refused call changes nothing.  GCM_ERR_ARG: a null handle, no parameters in
 * gcm_hdiff_step, order not 1 or 2, fields 0 or with unknown bits, nu not finite or <= 0, cmax outside (0, 1/8], a
 * non-finite dt, the probes' null pointers, H, W or nlev < 1, nout < GCM_HDIFF_PLAN_WORDS (message of the probes:
 * gcm_last_error(NULL)).  GCM_ERR_UNSUPPORTED: other models, a handle created with nranks > 1 that has not opted in,
 * W < 4 or, on a single domain, H < 4 (the radius-2 halo wraps once only).                                            */
#define GCM_HDIFF_U 1
#define GCM_HDIFF_V 2
#define GCM_HDIFF_T 4
#define GCM_HDIFF_Q 8
#define GCM_HDIFF_PLAN_WORDS 7
typedef struct {
    int32_t order;         /* 1: del-2, 2: del-4 */
    int32_t fields;        /* mask of GCM_HDIFF_* */
    double nu;             /* m^2/s (order 1), m^4/s (order 2) */
    double cmax;           /* the cap of the diffusion numbers, (0, 1/8] */
} gcm_hdiff;
int gcm_set_hdiff(gcm_handle *h, const gcm_hdiff *d);
int gcm_hdiff_on(const gcm_handle *h);
int gcm_hdiff_step(gcm_handle *h, double dt, const gcm_hdiff *d);
int gcm_hdiff_tables(int H, const double *dx_j, const double *dx_h, double dy, const gcm_hdiff *d, double dt, double *out);
int gcm_hdiff_apply(int H, int W, int nlev, const double *tab4, int order, const double *X, double *out);
int gcm_hdiff_apply_band(int Hb, int W, int nlev, const double *tab4, int order, const double *X, double *out);
int gcm_hdiff_plan(gcm_handle *h, int *out, int nout);
int gcm_set_band_hdiff(gcm_handle *h, int on);
int gcm_band_hdiff(const gcm_handle *h);
/* The end of a GCM_PE25D step whose dynamics the caller took itself: everything gcm_step and gcm_band_run queue behind
 * the corrector, in their order and by their code -- the horizontal diffusion (gcm_set_hdiff: a single domain's; a band's:
 * gcm_end_step_diffuse), the
 * solar step at the handle's clock, utc += dt, the Held-Suarez
 * forcing, the boundary layer, the convective adjustment, the moist physics (their sums, seconds and
 * nsteps advance as in gcm_step), the
 * climatology's step counter and its sample where one is due, then the spectra's step counter and sample (gcm_set_spectra)
 * -- each only if registered, on the handle's stream.  With
 * nothing registered it queues nothing.  On a single domain gcm_half_step(h, 0, dt), gcm_half_step(h, 1, dt),
 * gcm_end_step(h, dt) is gcm_step(h, 1, dt).  On a latitude band it ends a step driven through gcm_step_phase or
 * gcm_step_interior / gcm_step_boundary and the caller's own exchange: the launches take the ghost rows with the own
 * rows, as the explicit gcm_solar_step, gcm_held_suarez_step, gcm_convect_step and gcm_moist_step do, so the ghost rows
 * of the current state, and of the ground temperature, must be current (the post-corrector exchange unpacked).
 * gcm_step and gcm_band_run end their steps themselves: do not call it behind them.
 * gcm_end_step_begin and gcm_end_step_finish are its two parts, split behind the boundary layer.  begin: the tables for
 * dt, the solar step (the clock advances once), the Held-Suarez forcing over own rows and ghost rows, the boundary layer
 * (a band: over its own rows).  finish: the convective adjustment and the moist physics over own rows and ghost rows,
 * the climatology's step counter and sample, the spectra's step counter and sample.  On every handle begin followed by finish, with the same dt, is
 * gcm_end_step.  A band with the boundary layer registered (gcm_set_band_boundary_layer) moves the ghost rows of the
 * current state between the two -- gcm_halo_pack2, the transfer, gcm_halo_unpack2 -- and gcm_end_step itself refuses such
 * a band (GCM_ERR_STATE, the message names the two calls); on a single domain, or a band without the phase, nothing
 * needs to happen between them.
 * gcm_end_step_diffuse is the part ahead of gcm_end_step_begin: on a band with the horizontal diffusion registered
 * (gcm_set_band_hdiff) it queues the diffusion of the band's own rows, behind the unpack of the post-corrector exchange;
 * the caller then exchanges the current state (gcm_halo_pack2, the transfer, gcm_halo_unpack2) and calls
 * gcm_end_step_begin.  On every other GCM_PE25D handle it returns GCM_OK and queues nothing: a single domain keeps its
 * diffusion at the head of gcm_end_step_begin / gcm_end_step.  On such a band gcm_end_step is GCM_ERR_STATE, and so is
 * gcm_end_step_begin without a gcm_end_step_diffuse ahead of it for the step (the messages name the calls; a refused
 * call changes nothing).
 * Errors: a null handle GCM_ERR_ARG; other models GCM_ERR_UNSUPPORTED; a non-finite dt GCM_ERR_ARG, and nothing changes. */
int gcm_end_step(gcm_handle *h, double dt);
int gcm_end_step_diffuse(gcm_handle *h, double dt);
int gcm_end_step_begin(gcm_handle *h, double dt);
int gcm_end_step_finish(gcm_handle *h, double dt);

/* Device-side snapshot / restore of the current state, ghost rows included (2-D models): a long
 * run can restart from a known state without a host round trip.  gcm_restore is asynchronous on
 * the handle's stream.                                                                          */
int gcm_snapshot(gcm_handle *h);
int gcm_restore(gcm_handle *h);

/* Latitude-band ghost rows (nranks > 1).  The library packs the rows a neighbour
 * needs into / unpacks them from caller-owned DEVICE buffers (e.g. torch tensors
 * handed to torch.distributed / RCCL send-recv); it never calls a collective
 * itself.  `side` 0 = towards row 0 (north), 1 = towards the last row (south).
 * gcm_halo_bytes gives the buffer size for one side.  GCM_PE25D, segment by segment: the two rows of p,
 * then of u, v, t, q (every level) in the handle's storage type, then the two rows of the ground
 * temperature in float64 (see gcm_set_physics), then -- with n = gcm_set_band_tracers(n) > 0 -- the R rows
 * (every level) next to the boundary of each tracer in order, as one contiguous segment per tracer, in the storage
 * type; R = gcm_band_tracer_rows: 1 by default (the centred and the donor-cell scheme read rows j -+ 1 only), 2
 * after gcm_set_band_tracer_rows(h, 2).
 * Bytes per side:  esz 2 W (1 + 4 L) + 8 * 2 W + n esz R L W  (esz = 8 for fp64, 4 for fp32 storage).
 * Each message carries the tracers that belong to the state it carries (the predicted ones after a
 * predictor, the current ones otherwise).                                                       */
size_t gcm_halo_bytes(const gcm_handle *h);
int gcm_halo_pack(gcm_handle *h, int side, void *dev_buf, void *stream);
int gcm_halo_unpack(gcm_handle *h, int side, const void *dev_buf, void *stream);
/* both sides with one launch (buffers as above: north = side 0, south = side 1) */
int gcm_halo_pack2(gcm_handle *h, void *north_buf, void *south_buf, void *stream);
int gcm_halo_unpack2(gcm_handle *h, const void *north_buf, const void *south_buf, void *stream);
/* Step split for comm/compute overlap: rows that need no ghost data, then the rest. */
int gcm_step_interior(gcm_handle *h, double dt, void *stream);
int gcm_step_boundary(gcm_handle *h, double dt, void *stream);
/* GCM_PE25D bands, exchange hidden behind the update kernel's interior rows: each Euler stage is
 * split into "everything the neighbours wait for" and "the rest".  phase 0: predictor K1-K3 + the
 * update of the two edge rows on either side; gcm_halo_pack then packs the PREDICTED edge rows;
 * phase 1: predictor update of the interior rows (overlaps the exchange); gcm_halo_unpack fills the
 * predicted state's ghosts; phase 2 / 3: the same for the corrector (pack = the NEW state's edge
 * rows; phase 3 ends with the swap; unpack then fills the new current state's ghosts, which the
 * next step's phase 0 needs).  Before the first step the current state's ghosts must be exchanged
 * once (pack / unpack with no phase pending).                                                    */
int gcm_step_phase(gcm_handle *h, int phase, double dt, void *stream);
/* Optional: register the two DEVICE send buffers (gcm_halo_bytes each).  Phase 0 / 2 then update the
 * edge rows AND pack them into these buffers on the handle's second stream, concurrently with
 * whatever the caller queues next on `stream` (phase 1 / 3, the interior rows); no gcm_halo_pack
 * call is needed for those phases.  gcm_wait_edges makes a stream (the one the send is posted on)
 * wait for that pack.  NULL, NULL unregisters.                                                  */
int gcm_set_halo_buffers(gcm_handle *h, void *north_send, void *south_send);
/* A stream for the exchange, owned by the handle (created on first request): HIP maps streams onto a
 * few hardware queues and two streams on one queue run in order, so the library hands out one that
 * it has measured to run beside the handle's stream (and its internal second stream).            */
int gcm_comm_stream(gcm_handle *h, void **stream);
int gcm_wait_edges(gcm_handle *h, void *stream);

/* The whole band step inside the library: one call per run instead of ~16 per step from the host.
 * gcm_set_exchange hands the library what it needs to post the ghost-row exchange itself -- the
 * RCCL communicator, the two ring neighbours, the addresses of ncclSend / ncclRecv / ncclGroupStart /
 * ncclGroupEnd in the librccl.so the process already has loaded (the library does not link RCCL), and
 * four DEVICE buffers of gcm_halo_bytes() each.  With all four function pointers NULL the exchange is
 * a device-local copy (the band is its own neighbour on both sides: the periodic single domain;
 * tests and the one-GPU scaling tools).  gcm_band_run then runs `nsteps` full steps, exchanges
 * included (GCM_PE25D: two per step, posted on the handle's comm stream behind the edge rows and
 * overlapped with the interior rows; 2-D models: one per halo_steps steps), asynchronously on the
 * handle's streams.  The sequence is the one gcm_step_phase / gcm_halo_* document, so the results
 * are bit-identical to a host-driven band.                                                       */
typedef int (*gcm_p2p_fn)(const void *buf, size_t count, int datatype, int peer, void *comm, void *stream);
typedef int (*gcm_group_fn)(void);
typedef struct {
    void *comm;               /* ncclComm_t */
    int32_t north, south;     /* ranks of the ring neighbours in that communicator */
    gcm_p2p_fn send, recv;    /* ncclSend, ncclRecv   (bytes are sent as ncclChar) */
    gcm_group_fn group_start, group_end;
    void *send_north, *send_south, *recv_north, *recv_south;
} gcm_exchange;
int gcm_set_exchange(gcm_handle *h, const gcm_exchange *x);   /* NULL: unregister */
int gcm_band_run(gcm_handle *h, int nsteps, double dt);
/* 2-D models with halo_steps > 1 (an exchange every k steps): on = 1 hides the exchange behind the
 * interior rows of the step before and the step after it (the last step of a window produces, packs
 * and sends its edge rows first; the first step of the next starts with the rows that need no ghost
 * data).  Same kernels on the same rows: bit-identical results.  Costs four more launches per window,
 * so it pays where the exchange takes longer than that (measured per run by bench.py --gpus N, which
 * times both and keeps the faster).  Default off, or GCM_BAND_OVERLAP=1 at gcm_set_exchange.       */
/* GCM_PE25D bands: on = 1 holds the interior rows' update kernel back until the library's second stream has reached
 * the edge rows' update kernel, so that the edge rows' workgroups are dispatched first (15-20 us instead of the 60-70
 * they take when the two launches race for the chip): the pack and the exchange of a stage start ~45 us earlier, the
 * interior rows ~10 us later.  Same kernels on the same rows: bit-identical results.  Pays where an exchange takes
 * longer than ~30 us (measured per run by bench.py --gpus N, as above).  Default off.                              */
int gcm_set_band_overlap(gcm_handle *h, int on);

int gcm_sync(gcm_handle *h);

/* Stand-alone 2-D operators of two_d.py on velocity stacks V[axis] (host arrays in/out; V is
 * [2][H][W] with V[0] acting along array axis 0 = rows and dx0 = spatial_change[0], as
 * two_d.py:16-22).  `axes` is a bit mask (1 = axis 0, 2 = axis 1, 3 = both, axis 0 first --
 * the dimension split of corner_transport_2d / finite_volume_advection); `finite` = 1 returns
 * the increment of one axis pass instead of the new field (the *_finite functions).          */
typedef enum {
    GCM_ADV_UPWIND = 0,    /* upwind_axis / corner_transport_2d           two_d.py:11-71            */
    GCM_ADV_FV_UPWIND = 1, /* fv_advect_axis_upwind / finite_volume_advection  two_d.py:103-132,198-207 */
    GCM_ADV_FV_PLAIN = 2,  /* fv_advect_axis_plain                        two_d.py:135-166          */
    GCM_ADV_VANLEER = 3,   /* fv upwind + van_leer(calc_r)-limited centred flux (composition)        */
    GCM_ADV_MOMENTUM = 4   /* advect_with_momentum: V * pressure_at_edge(p), then fv upwind  :277-292 */
} gcm_adv_scheme;
int gcm_advect2d(int scheme, int axes, int finite, int width, int height, int nsteps, double dt,
                 double dx0, double dx1, const double *V, const double *q_in, double *q_out);
/* kind 0: pgf_c_grid_axis gradients (two_d.py:210-220); 1: pgf_c_grid (needs t, :223-245);
 * 2: pgf_templess (:248-261); 3: pressure_at_edge (:264-268; out2[0] alone is
 * pressure_at_edge_one_d, :271-274); 4: gradient, centred (:74-77); 5: pressure_gradient (needs t,
 * :80-100); 6: pgf_one_d along axis 0 in out2[0] and along axis 1 in out2[1] (:295-303; the edge
 * density is taken along axis 0 for either, as the reference does).  out2 is [2][H][W]; a 1-D array
 * of n cells is height n, width 1.                                                          */
int gcm_pgf2d(int kind, int width, int height, double dt, double dx0, double dx1, const double *p,
              const double *t, double *out2);
/* The 2-D operators the step kernels are fused from, one by one (host float64 arrays [H][W] in and
 * out, periodic in both axes as the reference's np.roll shifts): what matsuno_c_grid.py,
 * viscosity.py, matsumo_temp.py and temperature.py export.  Inputs x0, x1, x2 in the reference's
 * argument order; dx, mu where the operator takes them (else ignored).  The elementwise ones take
 * any array as height 1, width n.                                                            */
typedef enum {
    GCM_OP_ADV_U = 0,             /* advection_of_velocity_u(u, v, dx)        matsuno_c_grid.py:15-51  */
    GCM_OP_ADV_V = 1,             /* advection_of_velocity_v(u, v, dx)        :54-80                   */
    GCM_OP_GEO_GRAD_U = 2,        /* geopotential_gradient_u(p, dx)           :97-100                  */
    GCM_OP_GEO_GRAD_V = 3,        /* geopotential_gradient_v(p, dx)           :103-106                 */
    GCM_OP_ADV_GEO = 4,           /* advection_of_geopotential(u, v, p, dx)   :109-118                 */
    GCM_OP_LAPLACIAN = 5,         /* finite_laplacian_2d(q, dx)               viscosity.py:12-19       */
    GCM_OP_VISCOSITY = 6,         /* incompressible_viscosity_2d(u, mu, dx)   :22-25                   */
    GCM_OP_DENSITY_FROM = 7,      /* density_from(p, t)                       matsumo_temp.py:13-19    */
    GCM_OP_GEOPOTENTIAL_FROM = 8, /* geopotential_from(rho, p)                :45-47                   */
    GCM_OP_TO_TRUE_TEMP = 9,      /* to_true_temp(t, p)                       temperature.py:7-12      */
    GCM_OP_TO_POTENTIAL_TEMP = 10,/* to_potential_temp(tt, p)                 :15-19                   */
    GCM_OP_TO_DENSITY = 11,       /* to_density(tt, p)                        :22-24                   */
    GCM_OP_SCALING = 12,          /* scaling(pa, t, dx)                       matsumo_temp.py:28-30    */
    GCM_OP_UNSCALING = 13,        /* unscaling(pb, tt, dx)                    :33-35                   */
    GCM_OP_PE2D_ADVEC_P = 14,     /* advec_p(pu, pv, dx)                      no_limits_2d.py:41-44    */
    GCM_OP_PE2D_DUT = 15,         /* advec_m(p, u, v, dx)[0]                  :47-76                   */
    GCM_OP_PE2D_DVT = 16,         /* advec_m(p, u, v, dx)[1]                                           */
    GCM_OP_PE2D_PGF_U = 17,       /* pgf(p, t, dx)[0]                         :79-92                   */
    GCM_OP_PE2D_PGF_V = 18        /* pgf(p, t, dx)[1]                                                  */
} gcm_sw2d_op_kind;
int gcm_sw2d_op(int kind, int width, int height, double dx, double mu, const double *x0, const double *x1,
                const double *x2, double *out);
/* The operators of dynamics.py one by one (dynamics.py:15-181): host float64 arrays in the
 * reference's layout, 3-D [layers][height][width], 2-D [height][width], periodic in i and j (and in
 * k where the reference rolls k), geometry tables as geometry.gen_geometry builds them.  Inputs and
 * outputs in the reference's argument / return order:
 *   CALC_PU (p, u) -> pu            CALC_PV (p, v) -> pv         UN_PU (pu, p) -> u     UN_PV (pv, p) -> v
 *   AFLUX (pu, pv) -> pit[2-D], sd  ADVEC_SIG (sd, q) -> dq      ADVEC_M_PU (p, u, v, pu, pv) -> dut, dvt
 *   GEOPOTENTIAL (p, t) -> phi      PGF (p, t) -> pgfu, pgfv, phiu, phiv       ADVEC_T (pu, pv, t) -> dt   */
typedef enum {
    GCM_PEOP_CALC_PU = 0, GCM_PEOP_CALC_PV = 1, GCM_PEOP_UN_PU = 2, GCM_PEOP_UN_PV = 3, GCM_PEOP_AFLUX = 4,
    GCM_PEOP_ADVEC_SIG = 5, GCM_PEOP_ADVEC_M_PU = 6, GCM_PEOP_GEOPOTENTIAL = 7, GCM_PEOP_PGF = 8, GCM_PEOP_ADVEC_T = 9
} gcm_pe25d_op_kind;
typedef struct {
    const double *dx_j, *dx_h;                  /* [height]  geometry.py:136-137 */
    const double *dsig, *sig, *sigb, *sigt;     /* [layers]                      */
    const double *heightmap;                    /* [height][width] or NULL       */
    double dy, ptop;
} gcm_pe_geom;
int gcm_pe25d_op(int kind, int width, int height, int layers, const gcm_pe_geom *g, const double *const in[5],
                 double *const out[4]);
const char *gcm_pe25d_op_last_error(void);
/* flux_limiter.py on 1-D arrays of n cells (host arrays in/out; ip/im = np.roll by -1/+1,
 * coordinates_1d.py:25-30).  Results are BIT-identical to NumPy's, masks included: IEEE division,
 * no contraction.
 *   kind 0  van_leer(q)                    (r + |r|) / (1 + |r|)                       :10-11
 *   kind 1  calc_r(q)                      (q - im(q)) / (ip(q) - q), 0 where the denominator == 0  :14-20
 *   kind 2  donor_cell_flux(q, u)          where(u > 0, q, ip(q)) * u                  :23-27
 *   kind 3  donor_cell_advection(q,u,dx,dt) q + (im(flux) - flux) * dt / dx            :30-32
 * `u` is ignored by kinds 0 and 1 (may be NULL).                                                 */
typedef enum { GCM_FL_VAN_LEER = 0, GCM_FL_CALC_R = 1, GCM_FL_DONOR_FLUX = 2, GCM_FL_DONOR_ADVECTION = 3 } gcm_fl_kind;
int gcm_flux_limiter(int kind, int n, const double *q, const double *u, double dx, double dt, double *out);
/* The 1-D model of BASELINE configs[0] (no_limits.py:50-152): p, u, theta, q on a periodic line of n
 * cells, momentum form.  half_only = 1: ONE Euler stage, half_timestep(p,u,t,q, sp,su,st,sq, dt, dx)
 * (:115-147), base and stage given; half_only = 0: nsteps full Matsuno steps, matsuno_timestep
 * (:150-152), `stage` ignored.  Arrays are {p, u, t, q}, host float64.                            */
int gcm_pe1d(int n, int nsteps, int half_only, double dt, double dx, const double *const base[4],
             const double *const stage[4], double *const out[4]);
/* ... and its operators one by one (no_limits.py:50-112), arguments in the reference's order:
 * ADVEC_Q (u, q), CALC_PU (u, p), UN_PU (pu, p), ADVEC_P (pu), ADVEC_PU (p, pu, u), ADVEC_T (pu, t), PGF (p, t) */
typedef enum {
    GCM_OP1D_ADVEC_Q = 0, GCM_OP1D_CALC_PU = 1, GCM_OP1D_UN_PU = 2, GCM_OP1D_ADVEC_P = 3, GCM_OP1D_ADVEC_PU = 4,
    GCM_OP1D_ADVEC_T = 5, GCM_OP1D_PGF = 6
} gcm_pe1d_op_kind;
int gcm_pe1d_op(int kind, int n, double dx, const double *x0, const double *x1, const double *x2, double *out);
const char *gcm_ops_last_error(void);
/* The stand-alone operator entry points above (host arrays in, host arrays out: gcm_sw2d_op, gcm_pe25d_op,
 * gcm_pe1d_op, gcm_flux_limiter, gcm_pgf2d, gcm_advect2d) carve their device operands from a scratch arena the
 * calling thread keeps between calls (at most 256 MB: a call that needed more hands everything back when it
 * ends).  This frees the calling thread's arena now.  Returns 0.                                          */
int gcm_ops_release_scratch(void);

/* Timing helper for bench.py: runs nsteps steps bracketed by HIP events on the
 * handle's stream; returns elapsed milliseconds in *ms and, in *kernel_ms_avg,
 * the mean duration of the dominant kernel's launches measured by per-launch
 * event pairs in a second pass (so the first figure carries no event overhead).
 * NOTE: with kernel_ms_avg != NULL the state advances 2 * nsteps steps (the second
 * pass re-runs the same number of steps).  GCM_DIAG_ANY_NAN looks at u only, as the
 * reference's watch does (np.isnan(u).any(), matsuno_c_grid.py:184-187).            */
int gcm_time_steps(gcm_handle *h, int nsteps, double dt, double *ms, double *kernel_ms_avg);

#ifdef __cplusplus
}
#endif
#endif /* GCMCORE_H */

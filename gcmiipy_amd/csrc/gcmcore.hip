// Host side of libgcmcore.so: the C ABI of include/gcmcore.h -- create / destroy, state transfer, the 2-D step, ghost
// rows, snapshot / restore, members, gcm_sync, gcm_comm_stream, the band's step parts, gcm_half_step and gcm_time_steps.
// (gcm_band_run: gcm_band.hip; the reductions: gcm_diag.hip; what serves GCM_PE25D handles only, gcm_step's GCM_PE25D
// branch included: gcm_pe.hip.)  Owns device buffers, picks kernels, launches on the handle's stream.  There is
// no CPU fallback anywhere in this file: without a HIP device gcm_create fails.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "gcm_handle.h"

using namespace gcm;

std::string &gcm_create_error() {
    thread_local std::string e;
    return e;
}

static int alloc_field(gcm_handle *h, double **p) {
    // Every array starts a different multiple of 256 B past its (2 MiB-aligned) allocation: rows of a
    // power-of-two width would otherwise put the same (row, column) of all fields on the same HBM channel and
    // bank, and a wave of the fused kernel touches that element of ten arrays per row (tools/micro/copy_width.hip:
    // the bare access pattern moves 4-6 % faster with the arrays skewed).  GCM_ALLOC_SKEW=0 switches it off.
    // An ensemble's members follow one another at mstride elements (a whole number of 256-B lines, so that
    // every member's rows start as a single handle's do); the skew is per field, as for one member.  Sizes
    // in elements of esz bytes (fp32 handles: 4).
    static const long skew_unit = getenv("GCM_ALLOC_SKEW") ? atol(getenv("GCM_ALLOC_SKEW")) : 256;
    const size_t n = all_members_elems(h);
    const size_t skew = (size_t)(skew_unit > 0 ? skew_unit : 0) * (h->allocs.size() % 16) / h->esz;
    void *d = nullptr;
    HIPCHK(h, hipMalloc(&d, (n + skew) * h->esz));
    HIPCHK(h, hipMemsetAsync(d, 0, (n + skew) * h->esz, h->stream));
    h->allocs.push_back(d);
    *p = at(h, (double *)d, (long)(skew + (size_t)h->G * h->W));
    return GCM_OK;
}

// the Exner table of the models that carry a temperature, on the device
static bool upload_exner_table(gcm_handle *h) {
    double tab[kExnerTabDoubles];
    build_exner_table(tab);
    void *d = nullptr;
    if (hipMalloc(&d, sizeof tab) != hipSuccess) return false;
    h->allocs.push_back(d);
    h->exner_tab = (double *)d;
    return hipMemcpy(d, tab, sizeof tab, hipMemcpyHostToDevice) == hipSuccess;
}

extern "C" {

int gcm_abi_version(void) { return GCM_ABI_VERSION; }

int gcm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *gcm_build_info(void) {
    return "libgcmcore gfx950 (hipcc " __VERSION__ "), fp64, kernels: sw2d staged+fused, pe25d";
}

int gcm_exner_table(double *out256) {
    if (!out256) return GCM_ERR_ARG;
    build_exner_table(out256);
    return GCM_OK;
}

int gcm_filter_plan(int n, unsigned *out, int cap) { return pe25d_filter_plan(n, out, cap); }

const char *gcm_last_error(const gcm_handle *h) { return h ? h->err.c_str() : gcm_create_error().c_str(); }

int gcm_destroy(gcm_handle *h) {
    if (!h) return GCM_OK;
    if (h->cfg.device >= 0) (void)hipSetDevice(h->cfg.device);
    (void)hipStreamSynchronize(h->stream);
    if (h->comm) {
        (void)hipStreamSynchronize(h->comm);
        (void)hipStreamDestroy(h->comm);
    }
    if (h->pe) pe25d_destroy(h->pe);
    for (void *p : h->allocs) (void)hipFree(p);
    for (hipEvent_t e : h->time.ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->time.region) (void)hipEventDestroy(e);
    if (h->band.ev_pack) (void)hipEventDestroy(h->band.ev_pack);
    if (h->band.ev_comm) (void)hipEventDestroy(h->band.ev_comm);
    delete h;
    return GCM_OK;
}

int gcm_create(const gcm_config *cfg, gcm_handle **out) {
    if (!cfg || !out) return fail(nullptr, GCM_ERR_ARG, "gcm_create: null argument");
    *out = nullptr;
    if (cfg->abi_version != GCM_ABI_VERSION)
        return fail(nullptr, GCM_ERR_ARG, "gcm_create: abi_version mismatch");
    if (cfg->width < 1 || cfg->height < 1 || cfg->layers < 1)
        return fail(nullptr, GCM_ERR_ARG, "gcm_create: width/height/layers must be >= 1");
    if (cfg->nranks < 1 || cfg->rank < 0 || cfg->rank >= cfg->nranks)
        return fail(nullptr, GCM_ERR_ARG, "gcm_create: bad rank/nranks");
    const int hsteps = cfg->halo_steps < 1 ? 1 : cfg->halo_steps;
    if (cfg->nranks > 1 && cfg->height < kGhost * hsteps)
        return fail(nullptr, GCM_ERR_ARG, "gcm_create: a latitude band needs >= 2 * halo_steps rows");
    if (hsteps > 1 && (cfg->nranks == 1 || (cfg->model != GCM_SW2D && cfg->model != GCM_SW2D_TEMP)))
        return fail(nullptr, GCM_ERR_ARG, "gcm_create: halo_steps > 1 needs a 2-D latitude band");
    if (cfg->members < 0) return fail(nullptr, GCM_ERR_ARG, "gcm_create: members must be >= 0");
    if (cfg->members > 1 && cfg->model != GCM_SW2D && cfg->model != GCM_SW2D_TEMP)
        return fail(nullptr, GCM_ERR_UNSUPPORTED, "gcm_create: members > 1 needs GCM_SW2D or GCM_SW2D_TEMP");
    if (cfg->members > 1 && cfg->nranks > 1)
        return fail(nullptr, GCM_ERR_UNSUPPORTED, "gcm_create: members > 1 is not available on latitude bands");
    const bool sw2d = cfg->model == GCM_SW2D || cfg->model == GCM_SW2D_TEMP;
    if (sw2d && cfg->dtype != GCM_F64 && cfg->dtype != GCM_F32)
        return fail(nullptr, GCM_ERR_ARG, "gcm_create: bad dtype");
    // the ghost-row exchange copies 8-byte words (launch_seg_copy): G rows x (even W) floats is a whole number of them
    if (sw2d && cfg->dtype == GCM_F32 && cfg->nranks > 1 && cfg->width % 2)
        return fail(nullptr, GCM_ERR_UNSUPPORTED, "gcm_create: fp32 latitude bands need an even width");
    if (gcm_device_count() < 1)
        return fail(nullptr, GCM_ERR_NODEVICE,
                    "gcm_create: no HIP device visible; libgcmcore has no CPU fallback");
    gcm_handle *h = new gcm_handle;
    h->cfg = *cfg;
    h->W = cfg->width;
    h->H = cfg->height;
    h->L = cfg->layers;
    h->wrap = cfg->nranks == 1;
    h->G = kGhost * hsteps;
    h->M = cfg->members > 1 ? cfg->members : 1;
    h->f32 = sw2d && cfg->dtype == GCM_F32;
    h->esz = h->f32 ? 4 : 8;
    h->mstride = (long)(h->H + 2 * h->G) * h->W;
    const long line = 256 / h->esz;                      // elements per 256-B line
    if (h->M > 1) h->mstride = (h->mstride + line - 1) / line * line;
    h->stream = (hipStream_t)cfg->stream;
    int rc = GCM_OK;
    auto bail = [&](int code, const std::string &m) {
        gcm_create_error() = m.empty() ? h->err : m;
        gcm_destroy(h);
        return code;
    };
    if (cfg->device >= 0 && hipSetDevice(cfg->device) != hipSuccess)
        return bail(GCM_ERR_HIP, "gcm_create: hipSetDevice failed");

    switch (cfg->model) {
        case GCM_SW2D:
        case GCM_SW2D_TEMP: {
            if (!(cfg->dx > 0)) return bail(GCM_ERR_ARG, "gcm_create: dx must be > 0");
            const bool temp = cfg->model == GCM_SW2D_TEMP;
            if (!temp && cfg->tracer != GCM_TRACER_NONE)
                return bail(GCM_ERR_ARG, "gcm_create: tracer needs GCM_SW2D_TEMP");
            if (cfg->tracer < 0 || cfg->tracer > GCM_TRACER_VANLEER)
                return bail(GCM_ERR_ARG, "gcm_create: bad tracer");
            h->has[GCM_U] = h->has[GCM_V] = h->has[GCM_P] = true;
            h->has[GCM_T] = temp;
            h->has[GCM_Q] = temp && cfg->tracer != GCM_TRACER_NONE;
            h->variant = cfg->variant == GCM_VARIANT_AUTO ? GCM_VARIANT_FUSED : cfg->variant;
            if (h->variant != GCM_VARIANT_FUSED && h->variant != GCM_VARIANT_STAGED)
                return bail(GCM_ERR_ARG, "gcm_create: bad variant");
            for (int f = 0; f < GCM_NFIELDS; ++f) {
                if (!h->has[f]) continue;
                if ((rc = alloc_field(h, &h->cur[f]))) return bail(rc, "");
                if ((rc = alloc_field(h, &h->nxt[f]))) return bail(rc, "");
                if (f != GCM_Q && (rc = alloc_field(h, &h->star[f]))) return bail(rc, "");
            }
            if (temp) {
                if ((rc = alloc_field(h, &h->geo))) return bail(rc, "");
                if ((rc = alloc_field(h, &h->irho))) return bail(rc, "");
                if ((rc = alloc_field(h, &h->sst))) return bail(rc, "");
            }
            if (h->has[GCM_Q] && (rc = alloc_field(h, &h->qtmp))) return bail(rc, "");
            if (temp && !upload_exner_table(h)) return bail(GCM_ERR_HIP, "gcm_create: exner table upload failed");
            const int tr = h->has[GCM_Q] ? cfg->tracer : 0;
            if (h->f32) h->cols = sw2d_fused_cols<float>(h->W, h->H, temp, tr, h->wrap, h->M);   // 
            if (const char *e = getenv("GCM_SW2D_DEPTH"))   // (sw2d_fused_form; every other handle ignores it)
                if (temp && !h->f32 && (e[0] == '1' || e[0] == '3') && !e[1]) h->depth_pin = e[0] - '0';
            h->rows_per_band = h->f32 ? sw2d_fused_rows_per_band<float>(h->W, h->H, temp, tr, h->wrap, h->M, h->cols)
                                      : sw2d_fused_rows_per_band<double>(h->W, h->H, temp, tr, h->wrap, h->M, 1, h->depth_pin);
            // the wave pair (two steps per launch, sw2d_pair_kernel): its band length and its switch, for the handles
            // it can serve at all -- float64 GCM_SW2D_TEMP, fused, one member, a periodic single domain
            if (temp && !h->f32 && h->variant == GCM_VARIANT_FUSED && h->M == 1 && h->wrap) {
                if (const char *e = getenv("GCM_SW2D_PAIR"))
                    if ((e[0] == '0' || e[0] == '1') && !e[1]) h->pair_pin = e[0] - '0';
                const Sw2dFusedForm f = sw2d_fused_form(temp, tr, h->rows_per_band, h->W, h->H, h->M, h->esz, h->depth_pin);
                h->pair_rows = sw2d_pair_rows_per_band<double>(h->W, h->H, tr, f.stream);
            }
            break;
        }
        case GCM_PE2D: {
            if (!(cfg->dx > 0)) return bail(GCM_ERR_ARG, "gcm_create: dx must be > 0");
            if (cfg->nranks != 1)
                return bail(GCM_ERR_UNSUPPORTED, "gcm_create: GCM_PE2D has no latitude-band mode");
            h->variant = GCM_VARIANT_STAGED;
            for (int f = 0; f < GCM_NFIELDS; ++f) {
                h->has[f] = true;
                if ((rc = alloc_field(h, &h->cur[f]))) return bail(rc, "");
                if ((rc = alloc_field(h, &h->nxt[f]))) return bail(rc, "");
                if ((rc = alloc_field(h, &h->star[f]))) return bail(rc, "");
            }
            if (!upload_exner_table(h)) return bail(GCM_ERR_HIP, "gcm_create: exner table upload failed");
            break;
        }
        case GCM_PE25D: {
            std::string msg;
            h->pe = pe25d_create(*cfg, h->stream, &msg);
            if (!h->pe) return bail(msg.find("hip") == 0 ? GCM_ERR_HIP : GCM_ERR_ARG, msg);
            h->has[GCM_P] = h->has[GCM_U] = h->has[GCM_V] = h->has[GCM_T] = h->has[GCM_Q] = true;
            break;
        }
        default:
            return bail(GCM_ERR_UNSUPPORTED, "gcm_create: model not built in this round");
    }
    void *d = nullptr;
    if (hipMalloc(&d, sizeof(double) * 4 * diag_blocks_per_member(h) * h->M) != hipSuccess)
        return bail(GCM_ERR_HIP, "gcm_create: hipMalloc(diag) failed");
    h->allocs.push_back(d);
    h->diag_dev = (double *)d;
    if (hipStreamSynchronize(h->stream) != hipSuccess)
        return bail(GCM_ERR_HIP, "gcm_create: stream sync failed");
    *out = h;
    return GCM_OK;
}

// ------------------------------------------------------------------ state transfer
// member < 0: all members ([M][H][W] host arrays; the device slabs are mstride elements apart, so one 2-D copy
// per field), else that member alone ([H][W]).  fp32 handles: through a float64 staging buffer, one conversion
// launch per field and chunk of members (rounded to nearest-even up, widened exactly down).  The buffer holds
// as many members as fit 16 MB, at least one: it does not grow with the ensemble.
static int xfer(gcm_handle *h, double *const dev[GCM_NFIELDS], const double *const hostc[GCM_NFIELDS],
                double *const hostm[GCM_NFIELDS], bool to_device, int member = -1) {
    const size_t bytes = (size_t)h->H * h->W * sizeof(double), pitch = (size_t)h->mstride * sizeof(double);
    if (h->f32 && !h->staging) {
        const size_t fit = ((size_t)16 << 20) / bytes;
        h->staging_members = (int)std::max<size_t>(1, std::min<size_t>(fit, (size_t)h->M));
        void *d = nullptr;
        HIPCHK(h, hipMalloc(&d, bytes * h->staging_members));
        h->allocs.push_back(d);
        h->staging = (double *)d;
    }
    for (int f = 0; f < GCM_NFIELDS; ++f) {
        const void *src = hostc ? (const void *)hostc[f] : (const void *)hostm[f];
        if (!src) continue;
        if (!h->has[f] || !dev[f])
            return fail(h, GCM_ERR_ARG, "state transfer: field not part of this model");
        double *d = at(h, dev[f], (long)(member < 0 ? 0 : member) * h->mstride);
        if (h->f32) {
            const int nm = member < 0 ? h->M : 1;
            const long n = (long)h->H * h->W;
            // (each chunk's use of the staging buffer follows the previous one's in stream order)
            for (int m0 = 0; m0 < nm; m0 += h->staging_members) {
                const int k = std::min(h->staging_members, nm - m0);
                float *dm = (float *)at(h, d, (long)m0 * h->mstride);
                if (to_device) {
                    HIPCHK(h, hipMemcpyAsync(h->staging, hostc[f] + (size_t)m0 * n, bytes * k, hipMemcpyHostToDevice,
                                             h->stream));
                    launch_narrow(dm, h->mstride, h->staging, n, k, h->stream);
                } else {
                    launch_widen(h->staging, dm, h->mstride, n, k, h->stream);
                    HIPCHK(h, hipMemcpyAsync(hostm[f] + (size_t)m0 * n, h->staging, bytes * k, hipMemcpyDeviceToHost,
                                             h->stream));
                }
                HIPCHK(h, hipGetLastError());
            }
        } else if (member >= 0 || h->M == 1) {
            if (to_device)
                HIPCHK(h, hipMemcpyAsync(d, hostc[f], bytes, hipMemcpyHostToDevice, h->stream));
            else
                HIPCHK(h, hipMemcpyAsync(hostm[f], d, bytes, hipMemcpyDeviceToHost, h->stream));
        } else if (to_device) {
            HIPCHK(h, hipMemcpy2DAsync(d, pitch, hostc[f], bytes, bytes, h->M, hipMemcpyHostToDevice, h->stream));
        } else {
            HIPCHK(h, hipMemcpy2DAsync(hostm[f], bytes, d, pitch, bytes, h->M, hipMemcpyDeviceToHost, h->stream));
        }
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return GCM_OK;
}

int gcm_set_state(gcm_handle *h, const double *p, const double *u, const double *v,
                  const double *t, const double *q) {
    if (!h) return GCM_ERR_ARG;
    h->band.primed = false;                               // gcm_band_run: the new state's ghost rows are not exchanged yet
    h->ghosts_current = false;
    if (h->pe) return pe25d_set(h->pe, false, p, u, v, t, q, h->stream, &h->err);
    const double *src[GCM_NFIELDS] = {p, u, v, t, q};
    h->star_valid = false;
    return xfer(h, h->cur, src, nullptr, true);
}

int gcm_get_state(gcm_handle *h, double *p, double *u, double *v, double *t, double *q) {
    if (!h) return GCM_ERR_ARG;
    if (h->pe) return pe25d_get(h->pe, false, p, u, v, t, q, h->stream, &h->err);
    double *dst[GCM_NFIELDS] = {p, u, v, t, q};
    return xfer(h, h->cur, nullptr, dst, false);
}

int gcm_set_star(gcm_handle *h, const double *p, const double *u, const double *v,
                 const double *t, const double *q) {
    if (!h) return GCM_ERR_ARG;
    if (h->pe) return pe25d_set(h->pe, true, p, u, v, t, q, h->stream, &h->err);
    if (q && h->cfg.model != GCM_PE2D)
        return fail(h, GCM_ERR_ARG, "set_star: the tracer has no predicted state");
    const double *src[GCM_NFIELDS] = {p, u, v, t, q};     // (q: GCM_PE2D only, NULL otherwise)
    int rc = xfer(h, h->star, src, nullptr, true);
    if (rc == GCM_OK) h->star_valid = true;
    return rc;
}

int gcm_get_star(gcm_handle *h, double *p, double *u, double *v, double *t, double *q) {
    if (!h) return GCM_ERR_ARG;
    if (h->pe) return pe25d_get(h->pe, true, p, u, v, t, q, h->stream, &h->err);
    if (!h->star_valid) return fail(h, GCM_ERR_STATE, "get_star: no predicted state yet");
    if (q && h->cfg.model != GCM_PE2D)
        return fail(h, GCM_ERR_ARG, "get_star: the tracer has no predicted state");
    double *dst[GCM_NFIELDS] = {p, u, v, t, q};           // (q: GCM_PE2D only, NULL otherwise)
    return xfer(h, h->star, nullptr, dst, false);
}

// ------------------------------------------------------------------ stepping (2-D)
static Sw2dArgs base_args(gcm_handle *h, double dt) {
    Sw2dArgs a{};
    a.bu = h->cur[GCM_U];
    a.bv = h->cur[GCM_V];
    a.bp = h->cur[GCM_P];
    a.bt = h->cur[GCM_T];
    a.bq = h->cur[GCM_Q];
    a.exner_tab = h->exner_tab;
    a.W = h->W;
    a.H = h->H;
    a.wrap_j = h->wrap ? 1 : 0;
    a.j0 = 0;
    a.j1 = h->H;
    a.rows_per_band = h->rows_per_band;
    a.members = h->M;
    a.mstride = h->mstride;
    a.dt = dt;
    a.dx = h->cfg.dx;
    a.inv_dx = 1.0 / h->cfg.dx;
    a.dx2 = h->cfg.dx * h->cfg.dx;
    a.inv_dx2 = 1.0 / (h->cfg.dx * h->cfg.dx);
    a.h_dx = 0.5 / h->cfg.dx;
    a.dtdx = dt / h->cfg.dx;
    a.g_dx = 9.8 / h->cfg.dx;
    a.mu_dx2 = (18.5 * 1e-6) * 287.0 / (h->cfg.dx * h->cfg.dx);   // mu_air Rd / dx^2 (see thermo())
    a.inv_dx2_ = a.inv_dx2;
    return a;
}

// The 2-D launchers on the handle's real type: an fp32 handle's argument block is the same one, narrowed.
static void run_derive(const gcm_handle *h, const Sw2dArgs &a, hipStream_t s) {
    if (h->f32) launch_sw2d_derive(narrow_args(a), s);
    else launch_sw2d_derive(a, s);
}
static void run_stage(const gcm_handle *h, const Sw2dArgs &a, bool temp, hipStream_t s) {
    if (h->f32) launch_sw2d_stage(narrow_args(a), temp, s);
    else launch_sw2d_stage(a, temp, s);
}
static void run_tracer_axis(const gcm_handle *h, const Sw2dArgs &a, int axis, bool limit, const double *q_in,
                            double *q_out, hipStream_t s) {
    if (h->f32) launch_tracer_axis(narrow_args(a), axis, limit, (const float *)q_in, (float *)q_out, s);
    else launch_tracer_axis(a, axis, limit, q_in, q_out, s);
}
static bool run_fused(const gcm_handle *h, const Sw2dArgs &a, bool temp, int tracer, hipStream_t s) {
    return h->f32 ? launch_sw2d_fused(narrow_args(a), temp, tracer, s, h->cols) : launch_sw2d_fused(a, temp, tracer, s, 1, h->depth_pin);
}
static bool run_fused2(const gcm_handle *h, const Sw2dArgs &a, hipStream_t s) {
    return h->f32 ? launch_sw2d_fused2(narrow_args(a), s) : launch_sw2d_fused2(a, s);
}

// what the launches queued since the last check returned: the status hipLaunchKernel handed back for the
// fused step (kept in the handle: step_rows has many callers) and the runtime's sticky last error
int launch_status(gcm_handle *h) {
    const hipError_t e = hipGetLastError();
    if (h->launch_refused) {
        h->launch_refused = false;
        return fail(h, GCM_ERR_HIP, std::string("sw2d fused kernel: launch refused") +
                                        (e != hipSuccess ? std::string(": ") + hipGetErrorString(e) : std::string()));
    }
    HIPCHK(h, e);
    return GCM_OK;
}

void swap_state(gcm_handle *h) {
    for (int f = 0; f < GCM_NFIELDS; ++f) std::swap(h->cur[f], h->nxt[f]);
    h->ghosts_current = false;
}

static void tick(gcm_handle *h, hipStream_t s) {
    if (h->time.on && h->time.used < h->time.ev.size()) (void)hipEventRecord(h->time.ev[h->time.used++], s);
}

// predictor (stage 0) or corrector (stage 1) of the staged variant over rows [j0, j1)
static void staged_stage(gcm_handle *h, int stage, double dt, int j0, int j1, hipStream_t s) {
    if (h->cfg.model == GCM_PE2D) {
        launch_pe2d_stage(h->cur, stage == 0 ? h->cur : h->star, stage == 0 ? h->star : h->nxt,
                          h->exner_tab, h->W, h->H, dt, h->cfg.dx, s);
        return;
    }
    const bool temp = h->cfg.model == GCM_SW2D_TEMP;
    double *const *S = stage == 0 ? h->cur : h->star;
    double *const *O = stage == 0 ? h->star : h->nxt;
    Sw2dArgs a = base_args(h, dt);
    a.su = S[GCM_U];
    a.sv = S[GCM_V];
    a.sp = S[GCM_P];
    a.st = S[GCM_T];
    a.ou = O[GCM_U];
    a.ov = O[GCM_V];
    a.op = O[GCM_P];
    a.ot = O[GCM_T];
    a.j0 = j0;
    a.j1 = j1;
    if (temp) {
        Sw2dArgs d = a;
        d.dgeo = h->geo;
        d.dirho = h->irho;
        d.dst = h->sst;
        if (!h->wrap) {  // stencil reaches one row beyond the rows produced
            d.j0 = j0 - 1;
            d.j1 = j1 + 1;
        }
        run_derive(h, d, s);
        a.sgeo = h->geo;
        a.sirho = h->irho;
        a.sst = h->sst;
    }
    run_stage(h, a, temp, s);
}

static void staged_tracer(gcm_handle *h, double dt, int j0, int j1, hipStream_t s) {
    if (!h->has[GCM_Q] || h->cfg.model == GCM_PE2D) return;
    const bool lim = h->cfg.tracer == GCM_TRACER_VANLEER;
    Sw2dArgs a = base_args(h, dt);
    a.j0 = j0;
    a.j1 = j1;
    run_tracer_axis(h, a, 0, lim, h->cur[GCM_Q], h->qtmp, s);
    run_tracer_axis(h, a, 1, lim, h->qtmp, h->nxt[GCM_Q], s);
}

// one full Matsuno step producing rows [j0, j1) of nxt from cur (ghost rows already valid)
void step_rows(gcm_handle *h, double dt, int j0, int j1, hipStream_t s) {
    if (j1 <= j0) return;
    const bool temp = h->cfg.model == GCM_SW2D_TEMP;
    if (h->variant == GCM_VARIANT_FUSED) {
        Sw2dArgs a = base_args(h, dt);
        a.ou = h->nxt[GCM_U];
        a.ov = h->nxt[GCM_V];
        a.op = h->nxt[GCM_P];
        a.ot = h->nxt[GCM_T];
        a.oq = h->nxt[GCM_Q];
        a.j0 = j0;
        a.j1 = j1;
        tick(h, s);
        if (!run_fused(h, a, temp, h->has[GCM_Q] ? h->cfg.tracer : 0, s)) h->launch_refused = true;
        tick(h, s);
    } else {
        // the predicted state is needed one row beyond the rows produced
        const int e = h->wrap ? 0 : 1;
        staged_stage(h, 0, dt, j0 - e, j1 + e, s);
        tick(h, s);
        staged_stage(h, 1, dt, j0, j1, s);
        tick(h, s);
        staged_tracer(h, dt, j0, j1, s);
    }
}

// the argument block of a two-step launch: all rows of the (periodic) grid
static Sw2dArgs fused2_args(gcm_handle *h, double dt) {
    Sw2dArgs a = base_args(h, dt);
    a.ou = h->nxt[GCM_U];
    a.ov = h->nxt[GCM_V];
    a.op = h->nxt[GCM_P];
    a.j0 = 0;
    a.j1 = h->H;
    return a;
}

// Whether gcm_step takes its steps in pairs, two per launch (sw2d_fused2_kernel; small grids): plain shallow water,
// periodic rows, the fused variant, no per-launch timing, GCM_SW2D_TWO_STEP not 0 (read per call), and a geometry the
// two-step kernel serves.  Shared by gcm_step and gcm_sw2d_plan.
static bool steps_in_pairs(gcm_handle *h) {
    if (h->cfg.model != GCM_SW2D || !h->wrap || h->variant != GCM_VARIANT_FUSED || h->time.on) return false;
    if (getenv("GCM_SW2D_TWO_STEP") && getenv("GCM_SW2D_TWO_STEP")[0] == '0') return false;
    const Sw2dArgs a = fused2_args(h, 0.0);
    return sw2d_fused2_serves(a.wrap_j, a.j0, a.j1, a.H, a.rows_per_band);
}

// Whether gcm_step takes its steps in pairs through the wave pair (sw2d_pair_kernel): a handle it can serve
// (pair_rows: float64 GCM_SW2D_TEMP, fused, one member, periodic), no per-launch timing, and either GCM_SW2D_PAIR=1 or,
// with the switch unset, the default below.  Shared by gcm_step, gcm_sw2d_plan and gcm_sw2d_pair_info.
static bool steps_in_wave_pairs(gcm_handle *h) {
    if (h->pair_rows <= 0 || h->time.on) return false;
    if (!sw2d_pair_serves(h->wrap ? 1 : 0, 0, h->H, h->H, h->W, h->M, h->pair_rows)) return false;
    if (h->pair_pin >= 0) return h->pair_pin == 1;
    // the grids the deep march streams, the rule that picks depth 3: 0.77 of the single steps' time on C3
    const Sw2dFusedForm f = sw2d_fused_form(true, h->has[GCM_Q] ? h->cfg.tracer : 0, h->rows_per_band, h->W, h->H, h->M, h->esz, h->depth_pin);
    return f.stream && f.depth == 3;
}

static bool run_pair(gcm_handle *h, double dt) {
    const int tracer = h->has[GCM_Q] ? h->cfg.tracer : 0;
    Sw2dArgs a = fused2_args(h, dt);
    a.ot = h->nxt[GCM_T];
    a.oq = h->nxt[GCM_Q];
    a.rows_per_band = h->pair_rows;
    const Sw2dFusedForm f = sw2d_fused_form(true, tracer, h->rows_per_band, h->W, h->H, h->M, h->esz, h->depth_pin);
    return launch_sw2d_pair(a, tracer, f.stream, h->stream);
}

// the rows a band's next single step produces beyond its own, per side: each step consumes two ghost rows per side;
// the rows still valid shrink towards the interior until the next exchange (communication-avoiding deep halo)
static int step_extra_rows(const gcm_handle *h) { return h->wrap ? 0 : h->G - kGhost * (h->since_exchange + 1); }

int gcm_step(gcm_handle *h, int nsteps, double dt) {
    if (!h || nsteps < 0) return GCM_ERR_ARG;
    if (int rc = select_device(h)) return rc;
    if (h->pe) return pe_step(h, nsteps, dt);
    if (!h->wrap && h->since_exchange + nsteps > h->G / kGhost)
        return fail(h, GCM_ERR_STATE,
                    "gcm_step: a latitude band needs a ghost-row exchange every halo_steps steps");
    int n0 = 0;
    if (steps_in_pairs(h)) {
        while (nsteps - n0 >= 2) {
            // (the geometry is one the kernel serves: a refusal here is the runtime's, and an error)
            if (!run_fused2(h, fused2_args(h, dt), h->stream)) {
                h->launch_refused = true;
                return launch_status(h);
            }
            swap_state(h);
            n0 += 2;
        }
    } else if (steps_in_wave_pairs(h)) {
        for (; nsteps - n0 >= 2; n0 += 2) {
            if (!run_pair(h, dt)) {
                h->launch_refused = true;
                return launch_status(h);
            }
            swap_state(h);
        }
    }
    for (int n = n0; n < nsteps; ++n) {
        const int e = step_extra_rows(h);
        step_rows(h, dt, -e, h->H + e, h->stream);
        swap_state(h);
        if (!h->wrap) ++h->since_exchange;
    }
    h->star_valid = false;
    return launch_status(h);
}

// out: variant, rows per band, columns per lane, strip width of the single-step and of the two-step kernel, two-step
// launches, single steps, preloading form, STREAM form (include/gcmcore.h) -- from the expressions gcm_step and the
// launchers use themselves
int gcm_sw2d_plan(gcm_handle *h, int nsteps, int *out, int nout) {
    if (!h || h->pe || nsteps < 0 || !out || nout < GCM_SW2D_PLAN_WORDS) return GCM_ERR_ARG;
    const bool fused = h->variant == GCM_VARIANT_FUSED;
    const bool temp = h->cfg.model == GCM_SW2D_TEMP;
    const int pairs = steps_in_pairs(h) || steps_in_wave_pairs(h) ? nsteps / 2 : 0;
    const int e = step_extra_rows(h);
    Sw2dFusedForm f{false, false, 1};
    if (fused)
        f = sw2d_fused_form(temp, h->has[GCM_Q] ? h->cfg.tracer : 0, h->rows_per_band, h->W, h->H + 2 * e, h->M, h->esz, h->depth_pin);
    out[0] = h->variant;
    out[1] = fused ? h->rows_per_band : 0;
    out[2] = fused ? h->cols : 0;
    out[3] = fused ? sw2d_fused_strip_cols(h->cols) : 0;
    out[4] = fused ? kStrip2Cols : 0;
    out[5] = pairs;
    out[6] = nsteps - 2 * pairs;
    out[7] = f.preload;
    out[8] = f.stream;
    return GCM_OK;
}

// rows of requests a wave of the next step's fused launch keeps in flight (sw2d_fused_form), from the expression the
// launcher uses; 0: the staged variant
int gcm_sw2d_fused_depth(gcm_handle *h) {
    if (!h || h->pe) return GCM_ERR_ARG;
    if (h->variant != GCM_VARIANT_FUSED) return 0;
    const int e = step_extra_rows(h);
    return sw2d_fused_form(h->cfg.model == GCM_SW2D_TEMP, h->has[GCM_Q] ? h->cfg.tracer : 0, h->rows_per_band, h->W,
                           h->H + 2 * e, h->M, h->esz, h->depth_pin).depth;
}

// the wave pair of a 2-D handle: whether gcm_step's next call of two or more steps goes through it, and its own band
// length (0: a handle it never serves)
int gcm_sw2d_pair_info(gcm_handle *h, int *out, int nout) {
    if (!h || h->pe || !out || nout < GCM_SW2D_PAIR_WORDS) return GCM_ERR_ARG;
    out[0] = steps_in_wave_pairs(h) ? 1 : 0;
    out[1] = h->pair_rows;
    return GCM_OK;
}

int gcm_step_interior(gcm_handle *h, double dt, void *stream) {
    if (!h) return GCM_ERR_ARG;
    if (h->pe) return pe25d_step_part(h->pe, 0, dt, (hipStream_t)stream, &h->err);
    if (h->wrap) return fail(h, GCM_ERR_STATE, "step_interior: handle is not a latitude band");
    if (h->G != kGhost) return fail(h, GCM_ERR_STATE, "step_interior: halo_steps > 1 steps through gcm_step");
    step_rows(h, dt, kGhost, h->H - kGhost, (hipStream_t)stream);
    return launch_status(h);
}

int gcm_step_boundary(gcm_handle *h, double dt, void *stream) {
    if (!h) return GCM_ERR_ARG;
    if (h->pe) return pe25d_step_part(h->pe, 1, dt, (hipStream_t)stream, &h->err);
    if (h->wrap) return fail(h, GCM_ERR_STATE, "step_boundary: handle is not a latitude band");
    hipStream_t s = (hipStream_t)stream;
    if (h->H <= 2 * kGhost) {
        step_rows(h, dt, 0, h->H, s);
    } else {
        step_rows(h, dt, 0, kGhost, s);
        step_rows(h, dt, h->H - kGhost, h->H, s);
    }
    swap_state(h);
    h->star_valid = false;
    return launch_status(h);
}

int gcm_comm_stream(gcm_handle *h, void **stream) {
    if (!h || !stream) return GCM_ERR_ARG;
    if (!h->comm) {
        if (int rc = select_device(h)) return rc;
        h->comm = concurrent_stream(h->stream, h->pe ? pe25d_aux_stream(h->pe) : nullptr);
        if (!h->comm) return fail(h, GCM_ERR_HIP, "gcm_comm_stream: stream creation failed");
    }
    *stream = (void *)h->comm;
    return GCM_OK;
}

int gcm_half_step(gcm_handle *h, int stage, double dt) {
    if (!h || (stage != 0 && stage != 1)) return GCM_ERR_ARG;
    if (h->pe) return pe25d_half(h->pe, stage, dt, h->stream, &h->err);
    if (!h->wrap) return fail(h, GCM_ERR_UNSUPPORTED, "half_step on a latitude band");
    if (stage == 0) {
        staged_stage(h, 0, dt, 0, h->H, h->stream);
        h->star_valid = true;
    } else {
        if (!h->star_valid) return fail(h, GCM_ERR_STATE, "half_step(1) before half_step(0)");
        staged_stage(h, 1, dt, 0, h->H, h->stream);
        staged_tracer(h, dt, 0, h->H, h->stream);
        swap_state(h);
        h->star_valid = false;
    }
    return launch_status(h);
}

// ------------------------------------------------------------------ ghost rows
size_t gcm_halo_bytes(const gcm_handle *h) {
    if (!h) return 0;
    if (h->pe) return pe25d_halo_bytes(h->pe);
    int nf = 0;
    for (int f = 0; f < GCM_NFIELDS; ++f) nf += h->has[f];
    return (size_t)nf * h->G * h->W * h->esz;
}

// side 0: rows [0, G) <-> buffer (pack: they become the north neighbour's south ghost rows;
// unpack: buffer -> ghost rows [-G, 0)); side 1: rows [H-G, H) / ghost rows [H, H+G)
static int halo_segments(gcm_handle *h, bool pack, int side, void *dev_buf, SegCopy *c) {
    if (h->pe) return pe25d_halo_segments(h->pe, pack, side, dev_buf, c, &h->err);
    double *b = (double *)dev_buf;
    const long n = (long)h->G * h->W;                    // elements; SegCopy counts 8-byte words (fp32: even W)
    for (int f = 0; f < GCM_NFIELDS; ++f) {
        if (!h->has[f]) continue;
        double *edge = side == 0 ? h->cur[f] : at(h, h->cur[f], (long)(h->H - h->G) * h->W);
        double *ghost = side == 0 ? at(h, h->cur[f], -n) : at(h, h->cur[f], (long)h->H * h->W);
        c->src[c->nseg] = pack ? edge : b;
        c->dst[c->nseg] = pack ? b : ghost;
        c->n[c->nseg++] = n * h->esz / 8;
        b = at(h, b, n);
    }
    return GCM_OK;
}

static int halo_run(gcm_handle *h, bool pack, void *north, void *south, void *stream) {
    SegCopy c{};
    int rc = GCM_OK;
    if (north) rc = halo_segments(h, pack, 0, north, &c);
    if (rc == GCM_OK && south) rc = halo_segments(h, pack, 1, south, &c);
    if (rc != GCM_OK) return rc;
    if (!pack && !h->pe) {
        h->since_exchange = 0;
        if (south) h->ghosts_current = true;       // (the total variation reads the south ghost row only)
    }
    // GCM_PE25D: ghost rows filled on any stream but the library's second one (a host-driven exchange, gcm_band_run's
    // first exchange of a run): the next stage's second-stream work must follow THAT, not only the last update kernel
    if (!pack && h->pe && (hipStream_t)stream != pe25d_aux_stream(h->pe)) pe25d_fork_invalidate(h->pe);
    if (h->pe) pe25d_follow_tracers(h->pe, (hipStream_t)stream);   // (a band's tracer rows: hazard 3 of half_t)
    launch_seg_copy(c, (hipStream_t)stream);
    return launch_status(h);
}

int gcm_halo_pack(gcm_handle *h, int side, void *dev_buf, void *stream) {
    if (!h || !dev_buf || (side != 0 && side != 1)) return GCM_ERR_ARG;
    return halo_run(h, true, side == 0 ? dev_buf : nullptr, side == 1 ? dev_buf : nullptr, stream);
}

int gcm_halo_unpack(gcm_handle *h, int side, const void *dev_buf, void *stream) {
    if (!h || !dev_buf || (side != 0 && side != 1)) return GCM_ERR_ARG;
    return halo_run(h, false, side == 0 ? (void *)dev_buf : nullptr, side == 1 ? (void *)dev_buf : nullptr, stream);
}

// both sides in one launch
int gcm_halo_pack2(gcm_handle *h, void *north_buf, void *south_buf, void *stream) {
    if (!h || !north_buf || !south_buf) return GCM_ERR_ARG;
    return halo_run(h, true, north_buf, south_buf, stream);
}

int gcm_halo_unpack2(gcm_handle *h, const void *north_buf, const void *south_buf, void *stream) {
    if (!h || !north_buf || !south_buf) return GCM_ERR_ARG;
    return halo_run(h, false, (void *)north_buf, (void *)south_buf, stream);
}

// Device-side snapshot of the current state (2-D models): lets a long run restart from a known
// state without a host round trip (bench.py: the SURVEY's noise initial state lives for a few
// hundred steps only).  gcm_restore is asynchronous on the handle's stream.
int gcm_snapshot(gcm_handle *h) {
    if (!h) return GCM_ERR_ARG;
    if (h->pe) return fail(h, GCM_ERR_UNSUPPORTED, "gcm_snapshot: 2-D models only");
    const size_t n = all_members_elems(h);
    for (int f = 0; f < GCM_NFIELDS; ++f) {
        if (!h->has[f]) continue;
        if (!h->snap[f]) {
            void *d = nullptr;
            HIPCHK(h, hipMalloc(&d, n * h->esz));
            h->allocs.push_back(d);
            h->snap[f] = (double *)d;
        }
        HIPCHK(h, hipMemcpyAsync(h->snap[f], at(h, h->cur[f], -(long)h->G * h->W), n * h->esz,
                                 hipMemcpyDeviceToDevice, h->stream));
    }
    h->snap_since_exchange = h->since_exchange;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return GCM_OK;
}

int gcm_restore(gcm_handle *h) {
    if (!h) return GCM_ERR_ARG;
    if (h->pe) return fail(h, GCM_ERR_UNSUPPORTED, "gcm_restore: 2-D models only");
    const size_t n = all_members_elems(h);
    for (int f = 0; f < GCM_NFIELDS; ++f) {
        if (!h->has[f]) continue;
        if (!h->snap[f]) return fail(h, GCM_ERR_STATE, "gcm_restore: no snapshot taken");
        HIPCHK(h, hipMemcpyAsync(at(h, h->cur[f], -(long)h->G * h->W), h->snap[f], n * h->esz,
                                 hipMemcpyDeviceToDevice, h->stream));
    }
    h->since_exchange = h->snap_since_exchange;
    h->ghosts_current = false;
    h->star_valid = false;
    h->band.primed = false;         // gcm_band_run: exchange the restored state's ghost rows first
    return GCM_OK;
}

int gcm_sync(gcm_handle *h) {
    if (!h) return GCM_ERR_ARG;
    if (h->pe) pe25d_join_tracers(h->pe, h->stream);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return GCM_OK;
}

int gcm_members(const gcm_handle *h) { return h ? h->M : GCM_ERR_ARG; }

int gcm_set_member(gcm_handle *h, int m, const double *p, const double *u, const double *v, const double *t,
                   const double *q) {
    if (!h) return GCM_ERR_ARG;
    if (m < 0 || m >= h->M) return fail(h, GCM_ERR_ARG, "gcm_set_member: member out of range");
    if (h->pe) return gcm_set_state(h, p, u, v, t, q);
    h->band.primed = false;
    h->ghosts_current = false;
    h->star_valid = false;
    const double *src[GCM_NFIELDS] = {p, u, v, t, q};
    return xfer(h, h->cur, src, nullptr, true, m);
}

int gcm_get_member(gcm_handle *h, int m, double *p, double *u, double *v, double *t, double *q) {
    if (!h) return GCM_ERR_ARG;
    if (m < 0 || m >= h->M) return fail(h, GCM_ERR_ARG, "gcm_get_member: member out of range");
    if (h->pe) return gcm_get_state(h, p, u, v, t, q);
    double *dst[GCM_NFIELDS] = {p, u, v, t, q};
    return xfer(h, h->cur, nullptr, dst, false, m);
}

int gcm_time_steps(gcm_handle *h, int nsteps, double dt, double *ms, double *kernel_ms_avg) {
    if (!h || nsteps < 1 || !ms) return GCM_ERR_ARG;
    // the two region events are created once and kept in the handle (freed by gcm_destroy), so no
    // exit of this function leaks them.  NOTE: with kernel_ms_avg != NULL the state advances
    // 2 * nsteps steps (the per-launch pass re-runs the same number of steps).
    while (h->time.region.size() < 2) {
        hipEvent_t e;
        HIPCHK(h, hipEventCreate(&e));
        h->time.region.push_back(e);
    }
    const hipEvent_t e0 = h->time.region[0], e1 = h->time.region[1];
    HIPCHK(h, hipEventRecord(e0, h->stream));
    int rc = gcm_step(h, nsteps, dt);
    if (rc) return rc;
    HIPCHK(h, hipEventRecord(e1, h->stream));
    HIPCHK(h, hipEventSynchronize(e1));
    float t = 0;
    HIPCHK(h, hipEventElapsedTime(&t, e0, e1));
    *ms = t;
    if (kernel_ms_avg) {
        // second pass: one event pair around every launch of the dominant kernel
        const size_t need = 2 * (size_t)nsteps;
        while (h->time.ev.size() < need) {
            hipEvent_t e;
            HIPCHK(h, hipEventCreate(&e));
            h->time.ev.push_back(e);
        }
        h->time.used = 0;
        h->time.on = true;
        if (h->pe) pe25d_timing(h->pe, &h->time.ev, &h->time.used);
        rc = gcm_step(h, nsteps, dt);
        h->time.on = false;
        if (h->pe) pe25d_timing(h->pe, nullptr, nullptr);
        if (rc) return rc;
        HIPCHK(h, hipStreamSynchronize(h->stream));
        double tot = 0;
        int cnt = 0;
        for (size_t k = 0; k + 1 < h->time.used; k += 2) {
            float d = 0;
            HIPCHK(h, hipEventElapsedTime(&d, h->time.ev[k], h->time.ev[k + 1]));
            tot += d;
            ++cnt;
        }
        *kernel_ms_avg = cnt ? tot / cnt : 0.0;
    }
    return GCM_OK;
}

}  // extern "C"

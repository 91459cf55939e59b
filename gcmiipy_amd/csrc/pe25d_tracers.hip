// GCM_PE25D passive tracers, host side: the launches of a stage, the stream protocol that keeps them ordered, the
// storage, the entry points behind gcm_*tracer* and the tracers' part of a band's ghost-row message.  No kernel lives
// here (the device side: pe25d_tracer*.h); where a launch sits in a stage is the orchestration's business (pe25d_kernels.hip).
#include "pe25d_host.h"
#include "pe25d_tracer_force.h"
#include "pe25d_tracer_mix.h"
#include "pe25d_tracer_stats.h"

namespace gcm {

// "<fn>: <the HIP error>" and GCM_ERR_HIP, or GCM_OK
static int hip_status(hipError_t e, const char *fn, std::string *err) {
    if (e == hipSuccess) return GCM_OK;
    *err = std::string(fn) + ": " + hipGetErrorString(e);
    return GCM_ERR_HIP;
}

// ---------------------------------------------------------------- the launches of one stage
// The vertical mixing of the step (pe25d_tracer_mix.h) on `st` over own rows [a0, a1) and [b0, b1), for the mixed
// tracers.  The tables belong to one dt: a stage with another builds them again on the host (tracer_mixing_coeffs, the
// routine behind gcm_tracer_mixing_coeffs), rounds them to T and sends them in the arguments of small launches on `st`,
// into the buffer the last tables did not use.  A corrector launch on another stream of the same stage waits for
// that upload (ev_tab); the launches of the step before ended before this stage's could start (hazard 1).
template <typename T>
static void launch_mixing(Pe25d *m, T dt, hipStream_t st, int a0, int a1, int b0, int b1) {
    PeTracers::Mix &x = m->tr.mix;
    const int L = m->L;
    const double dtd = (double)dt;
    if (!x.built || dtd != x.dt_built) {
        std::vector<double> lo(L), w(L), g(L);
        std::vector<T> tab;
        std::string err;
        for (int f = 0; f < m->tr.n; ++f) {
            if (x.k[f].empty()) continue;
            // (K was checked at the registration: the routine refuses nothing here)
            (void)tracer_mixing_coeffs(L, m->dsig_host.data(), x.k[f].data(), dtd, lo.data(), w.data(), g.data(), &err);
            for (const std::vector<double> *v : {&lo, &w, &g})
                for (int k = 0; k < L; ++k) tab.push_back((T)(*v)[k]);
        }
        x.cur ^= 1;
        T *const dst = (T *)x.tab[x.cur];
        for (size_t at = 0; at < tab.size(); at += kTmFillMax)
            launch_tracer_mix_fill<T>(dst + at, tab.data() + at, (int)std::min<size_t>(kTmFillMax, tab.size() - at), st);
        if (x.ev_tab) (void)hipEventRecord(x.ev_tab, st);
        x.tab_stream = st;
        x.n_waited = 0;
        x.built = true;
        x.dt_built = dtd;
    }
    if (st != x.tab_stream && x.ev_tab && std::find(x.waited, x.waited + x.n_waited, st) == x.waited + x.n_waited) {
        (void)hipStreamWaitEvent(st, x.ev_tab, 0);
        if (x.n_waited < 4) x.waited[x.n_waited++] = st;
    }
    TracerMixArgsT<T> ma{};
    int entries = 0;
    for (int f = 0; f < m->tr.n; ++f)
        if (!x.k[f].empty()) ma.c[entries++] = (T *)tr_field(m, 0, f);
    ma.tab = (const T *)x.tab[x.cur];
    ma.W = m->W; ma.L = L;
    ma.j0 = a0; ma.n0 = a1 - a0; ma.jb0 = b0; ma.n1 = b1 - b0;
    launch_tracer_mix<T>(ma, entries, st);
}

// The passive tracers of one stage (pe25d_tracer.h) over rows [r0, r1) and [rb0, rb1): base = the current tracers,
// stage = the star set in the corrector, out = the star set in the predictor and the current set again in the
// corrector (each cell reads its base value only at itself: in place).  Chunks of 4, then 2, then 1 tracers, one
// launch per chunk size (blockIdx.y = chunk).  The handle's scheme picks the kernel: the centred one of
// pe25d_tracer.h (GCM_TRACER_NONE: nothing about the launch differs) or the limited march of pe25d_tracer_lim.h.
template <typename T>
void launch_tracers(Pe25d *m, const PeArgsT<T> &a, int stage_set, int out_set, hipStream_t st, int r0, int r1, int rb0, int rb1) {
    const int nrows = std::max(0, r1 - r0) + std::max(0, rb1 - rb0);
    if (nrows <= 0) return;
    const long stride = tr_stride(m);
    T *const cur = (T *)tr_field(m, 0, 0), *const star = (T *)tr_field(m, 1, 0);
    TracerArgsT<T> t{};
    t.p = a.p; t.pn = a.pn; t.sp = a.sp; t.sv = a.sv; t.spu = a.spu; t.pit = a.pit;
    t.inv_dxj = a.inv_dxj; t.dsig = a.dsig; t.inv_dsig = a.inv_dsig; t.sigb = a.sigb;
    t.c = cur;
    t.sc = stage_set == 2 ? star : cur;
    t.oc = out_set == 2 ? star : cur;
    t.tstride = stride;
    t.W = m->W; t.H = m->H; t.L = m->L; t.Hg = m->Hg; t.row0 = m->cfg.row0; t.wrap = a.wrap;
    t.j0 = r0; t.j1 = std::max(r0, r1); t.jb0 = rb0; t.jb1 = std::max(rb0, rb1);
    t.dt = a.dt; t.inv_dy = a.inv_dy;
    const bool same = t.sc == t.c;
    const long tiles = (long)((m->W + kTrCols - 1) / kTrCols) * ((nrows + kTrRows - 1) / kTrRows);
    const dim3 block(kTrCols * kTrRows);
    int done = 0;
    for (const int nc : {4, 2, 1}) {
        const int chunks = (m->tr.n - done) / nc;
        if (chunks == 0) continue;
        TracerArgsT<T> c = t;
        c.c += done * stride; c.sc += done * stride; c.oc += done * stride;
        const TracerKernel<T> kern = m->tr.scheme == GCM_TRACER_NONE ? tracer_kernel_for<T>(nc, same)
                                                                     : tracer_lim_kernel_for<T>(m->tr.scheme, nc, same);
        hipLaunchKernelGGL(kern, dim3((unsigned)((tiles + 7) / 8 * 8), (unsigned)chunks), block, 0, st, c);
        done += chunks * nc;
    }
    // the vertical mixing and then the forcing of the step, right behind the corrector on the same stream and own
    // rows: whatever follows the tracer launch -- the events of its callers (ev_tr_int, ev_tr), a band's pack -- is
    // queued behind these launches too
    const int a0 = std::clamp(r0, 0, m->H), a1 = std::clamp(r1, a0, m->H);
    const int b0 = std::clamp(rb0, 0, m->H), b1 = std::clamp(rb1, b0, m->H);
    if (out_set != 2 && m->tr.mix.n_mixed > 0) launch_mixing<T>(m, a.dt, st, a0, a1, b0, b1);
    if (out_set != 2 && m->tr.n_forced > 0) {
        const long row = (long)m->L * m->W;
        TracerForceArgsT<T> fa{};
        fa.off0 = a0 * row; fa.n0 = (a1 - a0) * row;
        fa.off1 = b0 * row; fa.n1 = (b1 - b0) * row;
        fa.dt = a.dt;
        int entries = 0;
        for (int f = 0; f < m->tr.n; ++f) {
            const PeTracers::Force &r = m->tr.force[f];
            if (!r.on) continue;
            TracerForceEntryT<T> &en = fa.e[entries++];
            en.c = (T *)tr_field(m, 0, f);
            en.emis = (const T *)r.emis;
            en.mask = r.mask;
            en.source = (T)r.source;
            en.fac = (T)std::exp(-r.decay * (double)a.dt);
            en.pin = (T)r.pin_value;
        }
        launch_tracer_force<T>(fa, entries, st);
    }
    m->tr.star = out_set == 2;
    if (m->aux && st == m->aux) m->tr.pending = true;
}
template void launch_tracers<double>(Pe25d *, const PeArgsT<double> &, int, int, hipStream_t, int, int, int, int);
template void launch_tracers<float>(Pe25d *, const PeArgsT<float> &, int, int, hipStream_t, int, int, int, int);

// ---------------------------------------------------------------- the stream protocol
// Why each launch sits where it does: stage_tracers, chain_b_head and update_edges in pe25d_kernels.hip.  Hazard 1: the
// next stage's K1 and K4 overwrite what a tracer launch still reads.  A launch on the second stream is followed in stream
// order (`pending`: the caller's stream has yet to join it, through ev_tr); a band's whole or interior launch may sit on
// another stream: ev_tr_int follows it (stage_tracers_launched), the next stage's streams wait for it where they do not
// carry it themselves (follow_last_tracers), the caller's stream joins it (pe25d_join_tracers).  Hazards 2 and 3 (the
// edge launch behind the unpack, the pack behind the edge launch) are stream order in update_edges; a pack or unpack the
// caller queues takes pe25d_follow_tracers.  Hazard 4 (single domains; pe25d_convect_tracers_rows): the tracers' convective
// mixing writes the current tracers on the caller's stream at the end of a step.  It joins the launches above first
// (pe25d_join_tracers), and the next stage's tracer launch on the second stream follows it because it invalidates the fork
// at the last K4 (pe25d_fork_invalidate): chain B then waits for the caller's stream's position, not for ev_k4.  The
// invalidation was chosen over an event of its own: no record, and nothing at all where no tracer has opted in.
bool last_tracers_in_flight(const Pe25d *m) { return m->tr.int_wait; }

void follow_last_tracers(Pe25d *m, hipStream_t st) {
    m->tr.int_wait = false;
    if (st != m->tr.int_stream) (void)hipStreamWaitEvent(st, m->tr.ev_tr_int, 0);
}

void stage_tracers_launched(Pe25d *m, hipStream_t st, bool caller_joins) {
    (void)hipEventRecord(m->tr.ev_tr_int, st);
    m->tr.int_stream = st;
    m->tr.int_wait = true;
    if (caller_joins) m->tr.int_join = true;
}

void pe25d_join_tracers(Pe25d *m, hipStream_t s) {
    if (m->tr.int_join) {                                        // (a band's interior rows on the third stream)
        m->tr.int_join = false;
        if (m->tr.int_stream != s) (void)hipStreamWaitEvent(s, m->tr.ev_tr_int, 0);
    }
    if (!m->tr.pending) return;
    m->tr.pending = false;
    (void)hipEventRecord(m->tr.ev_tr, m->aux);
    (void)hipStreamWaitEvent(s, m->tr.ev_tr, 0);
}

// a ghost-row pack or unpack the caller queues on `s` (gcm_halo_pack / unpack): it follows the tracer launches on
// the second stream, which read the edge and ghost rows it moves.  (The interior rows on the third stream touch
// neither.)  Unlike pe25d_join_tracers this leaves the caller's join to come in place.
void pe25d_follow_tracers(Pe25d *m, hipStream_t s) {
    if (!m->tr.pending || s == m->aux) return;
    (void)hipEventRecord(m->tr.ev_tr, m->aux);
    (void)hipStreamWaitEvent(s, m->tr.ev_tr, 0);
}

// ---------------------------------------------------------------- storage
// forget the forcing of tracer f (f < 0: of every tracer) and free its fields; the caller has made sure that no launch
// still reads them
static void drop_tracer_forcing(Pe25d *m, int f) {
    for (int i = f < 0 ? 0 : f; i < (f < 0 ? GCM_MAX_TRACERS : f + 1); ++i) {
        PeTracers::Force &r = m->tr.force[i];
        if (r.emis_alloc) (void)hipFree(r.emis_alloc);
        if (r.mask_alloc) (void)hipFree(r.mask_alloc);
        if (r.on) --m->tr.n_forced;
        r = PeTracers::Force{};
    }
}

// forget the mixing of tracer f (f < 0: of every tracer); the tables are built anew at the next launch
static void drop_tracer_mixing(Pe25d *m, int f) {
    PeTracers::Mix &x = m->tr.mix;
    for (int i = f < 0 ? 0 : f; i < (f < 0 ? GCM_MAX_TRACERS : f + 1); ++i) {
        if (!x.k[i].empty()) --x.n_mixed;
        x.k[i].clear();
    }
    x.built = false;
}

// the fields, their forcing and their mixing go (no launch still reads them): the handle is without tracers
static hipError_t tracers_free(Pe25d *m) {
    const hipError_t e = m->tr.buf ? hipFree(m->tr.buf) : hipSuccess;
    m->tr.buf = nullptr; m->tr.n = 0; m->tr.star = false;
    drop_tracer_forcing(m, -1);                  // (the fields' placement followed the tracers' storage)
    drop_tracer_mixing(m, -1);                   // (the same life cycle)
    tracers_convect_forget(m);                   // (and the opt-ins of the convective mixing)
    return e;
}

// The tracers' storage anew: n fields a set with `rows` ghost rows a side on a band, zeros.  Joins the tracer streams
// and synchronises first; the count and the depth change together with the storage, or -- on a HIP error -- the handle
// is left without tracers at the depth asked for
static int tracers_alloc(Pe25d *m, int n, int rows, hipStream_t s, const char *fn, std::string *err) {
    PeTracers &t = m->tr;
    pe25d_join_tracers(m, s);
    hipError_t e = hipStreamSynchronize(s);
    const hipError_t freed = tracers_free(m);
    if (e == hipSuccess) e = freed;
    t.rows = rows;
    if (e == hipSuccess && n > 0) {
        const size_t bytes = 2 * (size_t)n * tr_stride(m) * elem_size(m);
        e = hipMalloc(&t.buf, bytes);
        if (e == hipSuccess) e = hipMemsetAsync(t.buf, 0, bytes, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);        // (whichever stream reads the fields first finds the zeros)
        for (hipEvent_t *ev : {&t.ev_tr, &t.ev_tr_int})
            if (e == hipSuccess && m->aux && !*ev) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    }
    if (e == hipSuccess) t.n = n;
    else (void)tracers_free(m);
    return hip_status(e, fn, err);
}

void tracers_destroy(Pe25d *m) {
    if (m->tr.ev_tr) (void)hipEventDestroy(m->tr.ev_tr);
    if (m->tr.ev_tr_int) (void)hipEventDestroy(m->tr.ev_tr_int);
    if (m->tr.mix.ev_tab) (void)hipEventDestroy(m->tr.mix.ev_tab);
    (void)tracers_free(m);
}

// gcm_set_band_tracers: a band's tracer count, fixed before the message size is used (zeros until gcm_set_tracers)
int pe25d_set_band_tracers(Pe25d *m, int n, hipStream_t s, std::string *err) {
    if (m->wrap) {
        *err = "gcm_set_band_tracers: GCM_PE25D latitude bands only (a single domain takes gcm_set_tracers directly)";
        return GCM_ERR_UNSUPPORTED;
    }
    if (n < 0 || n > GCM_MAX_TRACERS) { *err = "gcm_set_band_tracers: n must be 0 .. GCM_MAX_TRACERS"; return GCM_ERR_ARG; }
    if (m->halo_fixed) {
        *err = "gcm_set_band_tracers: send or exchange buffers are registered already (their size follows the count)";
        return GCM_ERR_STATE;
    }
    return tracers_alloc(m, n, m->tr.rows, s, "gcm_set_band_tracers", err);
}

// gcm_set_band_tracer_rows: the ghost rows a side of a band's tracers, fixed before the message size is used like
// the count.  A change of depth moves interior row 0 of every field: the tracers are allocated anew, as zeros
int pe25d_set_band_tracer_rows(Pe25d *m, int rows, hipStream_t s, std::string *err) {
    if (m->wrap) {
        *err = "gcm_set_band_tracer_rows: GCM_PE25D latitude bands only (a single domain's rows wrap: no ghost rows)";
        return GCM_ERR_UNSUPPORTED;
    }
    if (rows < 1 || rows > kTrGhostMax) {
        *err = "gcm_set_band_tracer_rows: rows must be 1 .. " + std::to_string(kTrGhostMax);
        return GCM_ERR_ARG;
    }
    if (m->halo_fixed) {
        *err = "gcm_set_band_tracer_rows: send or exchange buffers are registered already (their size follows the depth)";
        return GCM_ERR_STATE;
    }
    if (rows == m->tr.rows) return GCM_OK;
    if (rows < 2 && m->tr.scheme == GCM_TRACER_VANLEER) {
        *err = "gcm_set_band_tracer_rows: GCM_TRACER_VANLEER is in force and reads two ghost rows per side "
               "(gcm_set_tracer_scheme first)";
        return GCM_ERR_STATE;
    }
    return tracers_alloc(m, m->tr.n, rows, s, "gcm_set_band_tracer_rows", err);
}

int pe25d_band_tracer_rows(const Pe25d *m) { return tr_ghost(m); }
int pe25d_tracer_count(const Pe25d *m) { return m->tr.n; }
int pe25d_tracer_scheme(const Pe25d *m) { return m->tr.scheme; }

// gcm_set_tracer_scheme: between steps, with or without tracers.  The scheme is read where a stage launches its
// tracer kernels; the star tracers of an earlier predictor belong to the earlier scheme and are dropped.
int pe25d_set_tracer_scheme(Pe25d *m, int scheme, hipStream_t s, std::string *err) {
    // (a single domain's rows wrap through Idx; a band addresses rows j -+ 2 in its ghost rows, and the edge launch of
    // update_edges -- own rows [0, 2) and [H - 2, H) -- is the only one that reaches them)
    if (scheme == GCM_TRACER_VANLEER && !m->wrap && tr_ghost(m) < 2) {
        *err = "gcm_set_tracer_scheme: GCM_TRACER_VANLEER reads two rows either side of a cell, and this latitude band's "
               "tracers carry one ghost row per side (the message format of gcm_set_band_tracers); declare two with "
               "gcm_set_band_tracer_rows(h, 2) before the send or exchange buffers are registered";
        return GCM_ERR_UNSUPPORTED;
    }
    pe25d_join_tracers(m, s);
    m->tr.scheme = scheme;
    m->tr.star = false;
    return GCM_OK;
}

// gcm_set_tracers: the values of the current set.  A single domain's count follows n (another count: new storage, and
// the forcing goes with the tracers it belonged to; the same count keeps both); a band's was declared
int pe25d_set_tracers(Pe25d *m, int n, const double *c, hipStream_t s, std::string *err) {
    if (!m->wrap && m->tr.n == 0) {
        *err = "gcm_set_tracers: this latitude band declared no tracers (gcm_set_band_tracers)";
        return GCM_ERR_UNSUPPORTED;
    }
    if (!m->wrap && n != m->tr.n) {
        *err = "gcm_set_tracers: this latitude band declared " + std::to_string(m->tr.n) +
               " tracers (gcm_set_band_tracers); n must equal that";
        return GCM_ERR_ARG;
    }
    if (n < 0 || n > GCM_MAX_TRACERS || (n > 0 && !c)) {
        *err = "gcm_set_tracers: n must be 0 .. GCM_MAX_TRACERS, with a host array for n > 0";
        return GCM_ERR_ARG;
    }
    hipError_t e = hipSuccess;
    if (n != m->tr.n) {
        if (const int rc = tracers_alloc(m, n, m->tr.rows, s, "gcm_set_tracers", err)) return rc;
    } else {
        pe25d_join_tracers(m, s);
        e = hipStreamSynchronize(s);             // (the last tracer launch has ended: the fields are free to take)
    }
    const size_t cells = (size_t)m->H * m->L * m->W;
    for (int f = 0; f < n && e == hipSuccess; ++f) e = field_to_device(m, tr_field(m, 0, f), c + (size_t)f * cells, m->L, s);
    // the star set starts as a copy (a corrector behind gcm_set_star, without a predictor, reads it); a band's ghost
    // rows come with it, until the next exchange fills them
    const size_t set_bytes = (size_t)n * tr_stride(m) * elem_size(m);
    if (e == hipSuccess && n > 0) e = hipMemcpyAsync((char *)m->tr.buf + set_bytes, m->tr.buf, set_bytes, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    m->tr.star = false;
    pe25d_fork_invalidate(m);                    // (the uploads on the caller's stream: the next chain B follows them)
    return hip_status(e, "gcm_set_tracers", err);
}

int pe25d_get_tracers(Pe25d *m, int which, double *c, hipStream_t s, std::string *err) {
    if (which != 0 && which != 1) { *err = "gcm_get_tracers: which must be 0 (current) or 1 (star)"; return GCM_ERR_ARG; }
    if (which == 1 && !m->tr.star) { *err = "gcm_get_tracers: no predicted tracers yet"; return GCM_ERR_STATE; }
    if (m->tr.n > 0 && !c) { *err = "gcm_get_tracers: no host array"; return GCM_ERR_ARG; }
    pe25d_join_tracers(m, s);
    const size_t cells = (size_t)m->H * m->L * m->W;
    hipError_t e = hipSuccess;
    for (int f = 0; f < m->tr.n && e == hipSuccess; ++f) e = field_to_host(m, c + (size_t)f * cells, tr_field(m, which, f), m->L, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return hip_status(e, "gcm_get_tracers", err);
}

// ---------------------------------------------------------------- forcing
// a host field [k][j][i] in the device layout [j][k][i], narrowed to D
template <typename D, typename S>
static void to_device_layout(D *dst, const S *src, size_t W, size_t H, size_t L) {
    for (size_t j = 0; j < H; ++j)
        for (size_t k = 0; k < L; ++k)
            for (size_t i = 0; i < W; ++i) dst[(j * L + k) * W + i] = (D)src[(k * H + j) * W + i];
}

// gcm_set_tracer_forcing: f == nullptr clears tracer `tracer` (-1: all).  Includes the tracer stream and synchronises
// `s` first: no launch reads the fields that are replaced.  The new fields are allocated and filled before anything
// of the handle changes, so a refused or failed call changes nothing.  The host arrays [L][H][W] are reordered to the
// device layout [j][k][i] here (once per registration), the emission narrowed to the handle's real type.
int pe25d_set_tracer_forcing(Pe25d *m, int tracer, const gcm_tracer_forcing *f, hipStream_t s, std::string *err) {
    const bool clear_all = !f && tracer == -1;
    if (!clear_all && (tracer < 0 || tracer >= m->tr.n)) {
        *err = "gcm_set_tracer_forcing: tracer must be 0 .. gcm_tracer_count - 1 (or -1 without a record: clear all)";
        return GCM_ERR_ARG;
    }
    if (f && (!std::isfinite(f->source) || !std::isfinite(f->decay) || !std::isfinite(f->pin_value) || f->decay < 0.0)) {
        *err = "gcm_set_tracer_forcing: source, decay and pin_value must be finite, decay >= 0";
        return GCM_ERR_ARG;
    }
    pe25d_join_tracers(m, s);
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_status(e, "gcm_set_tracer_forcing", err);
    if (!f) {
        drop_tracer_forcing(m, tracer);
        return GCM_OK;
    }
    const size_t esz = elem_size(m);
    const size_t W = m->W, H = m->H, L = m->L, cells = W * H * L;
    const uintptr_t c0 = (uintptr_t)tr_field(m, 0, tracer);
    PeTracers::Force r;
    r.on = true;
    r.source = f->source; r.decay = f->decay; r.pin_value = f->pin_value;
    std::vector<unsigned char> host;
    if (f->emission) {
        host.resize(cells * esz);
        if (m->f32) to_device_layout((float *)host.data(), f->emission, W, H, L);
        else to_device_layout((double *)host.data(), f->emission, W, H, L);
        e = hipMalloc(&r.emis_alloc, cells * esz + 16);
        if (e == hipSuccess) {
            r.emis = (char *)r.emis_alloc + (c0 & 15);           // (hipMalloc aligns to 16 bytes and more)
            e = hipMemcpy(r.emis, host.data(), cells * esz, hipMemcpyHostToDevice);
        }
    }
    if (e == hipSuccess && f->pin_mask) {
        host.resize(cells);
        to_device_layout(host.data(), f->pin_mask, W, H, L);
        e = hipMalloc(&r.mask_alloc, cells + 16);
        if (e == hipSuccess) {
            r.mask = (unsigned char *)r.mask_alloc + ((c0 / esz) & (16 / esz - 1));
            e = hipMemcpy(r.mask, host.data(), cells, hipMemcpyHostToDevice);
        }
    }
    if (e != hipSuccess) {
        if (r.emis_alloc) (void)hipFree(r.emis_alloc);
        if (r.mask_alloc) (void)hipFree(r.mask_alloc);
        return hip_status(e, "gcm_set_tracer_forcing", err);
    }
    drop_tracer_forcing(m, tracer);
    m->tr.force[tracer] = r;
    ++m->tr.n_forced;
    return GCM_OK;
}

int pe25d_tracer_forced(const Pe25d *m, int tracer) {
    if (tracer < 0 || tracer >= m->tr.n) return GCM_ERR_ARG;
    return m->tr.force[tracer].on ? 1 : 0;
}

// ---------------------------------------------------------------- vertical mixing
// gcm_set_tracer_mixing: k == nullptr clears tracer `tracer` (-1: all).  Includes the tracer stream and synchronises
// `s` first, as the forcing does: no launch reads the tables that go out of use.  Everything is checked, and the two
// table buffers and their event exist, before anything of the handle changes: a refused or failed call changes nothing.
// The handle keeps K in float64; the tables follow at the next corrector (launch_mixing)
int pe25d_set_tracer_mixing(Pe25d *m, int tracer, const double *k, int nk, hipStream_t s, std::string *err) {
    const bool clear_all = !k && tracer == -1;
    if (!clear_all && (tracer < 0 || tracer >= m->tr.n)) {
        *err = "gcm_set_tracer_mixing: tracer must be 0 .. gcm_tracer_count - 1 (or -1 without a profile: clear all)";
        return GCM_ERR_ARG;
    }
    if (k) {
        if (m->L < 2) { *err = "gcm_set_tracer_mixing: one level has no interface to mix across (layers must be 2 or more)"; return GCM_ERR_ARG; }
        if (nk != m->L - 1) {
            *err = "gcm_set_tracer_mixing: nk must be layers - 1 = " + std::to_string(m->L - 1) + " (K at the interfaces between levels)";
            return GCM_ERR_ARG;
        }
        // (the routine's own checks: the same refusals, before anything changes)
        std::vector<double> lo(m->L), w(m->L), g(m->L);
        std::string why;
        if (tracer_mixing_coeffs(m->L, m->dsig_host.data(), k, 0.0, lo.data(), w.data(), g.data(), &why) != GCM_OK) {
            *err = "gcm_set_tracer_mixing: K must be finite and >= 0 at every interface";
            return GCM_ERR_ARG;
        }
    }
    pe25d_join_tracers(m, s);
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_status(e, "gcm_set_tracer_mixing", err);
    if (!k) {
        drop_tracer_mixing(m, tracer);
        return GCM_OK;
    }
    PeTracers::Mix &x = m->tr.mix;
    const size_t tab_bytes = (size_t)GCM_MAX_TRACERS * 3 * m->L * elem_size(m);
    for (void *&t : x.tab)
        if (!t && !dev_upload<char>(m, (char **)&t, nullptr, tab_bytes)) {
            *err = "hip: gcm_set_tracer_mixing allocation failed";
            return GCM_ERR_HIP;
        }
    if (!x.ev_tab && (e = hipEventCreateWithFlags(&x.ev_tab, hipEventDisableTiming)) != hipSuccess)
        return hip_status(e, "gcm_set_tracer_mixing", err);
    if (x.k[tracer].empty()) ++x.n_mixed;
    x.k[tracer].assign(k, k + nk);
    x.built = false;
    return GCM_OK;
}

int pe25d_tracer_mixed(const Pe25d *m, int tracer) {
    if (tracer < 0 || tracer >= m->tr.n) return GCM_ERR_ARG;
    return m->tr.mix.k[tracer].empty() ? 0 : 1;
}

// ---------------------------------------------------------------- monitor
// gcm_tracer_stats: the records of the tracers of set `which` (0 current, 1 star), then -- with_q -- of q of the same
// state set, over the band's own rows; mass and air take p of that state set.  Includes the tracer stream, two
// launches and one synchronisation of `s`; 48 bytes a field come back.  The buffers live in the handle.
int pe25d_tracer_stats(Pe25d *m, int which, bool with_q, double *out, int cap, hipStream_t s, std::string *err) {
    if (which != 0 && which != 1) { *err = "gcm_tracer_stats: which must be 0 (current) or 1 (star)"; return GCM_ERR_ARG; }
    const int nf = m->tr.n + (with_q ? 1 : 0);
    if (cap < GCM_TRACER_STATS_WORDS * nf) {
        *err = "gcm_tracer_stats: out holds " + std::to_string(cap) + " doubles, " + std::to_string(GCM_TRACER_STATS_WORDS * nf) +
               " are needed (GCM_TRACER_STATS_WORDS per tracer, and for q)";
        return GCM_ERR_ARG;
    }
    // the tracers' rule is gcm_get_tracers', q's is gcm_get_star's (without tracers and with q only the latter is left)
    if (which == 1 && !m->tr.star && (m->tr.n > 0 || !with_q)) { *err = "gcm_tracer_stats: no predicted tracers yet"; return GCM_ERR_STATE; }
    if (which == 1 && with_q && !m->star_valid) { *err = "gcm_tracer_stats: no predicted state yet"; return GCM_ERR_STATE; }
    if (nf == 0) return GCM_OK;
    const int groups = tracer_stats_groups(m->H, m->W);
    const size_t n_out = (size_t)GCM_TRACER_STATS_WORDS * (GCM_MAX_TRACERS + 1);
    if (!m->tr.stats_dev) {
        std::vector<double> init((size_t)m->L + n_out * (1 + (size_t)groups), 0.0);
        std::copy(m->dsig_host.begin(), m->dsig_host.end(), init.begin());
        if (!dev_upload<double>(m, &m->tr.stats_dev, init.data(), init.size())) {
            *err = "hip: gcm_tracer_stats allocation failed";
            return GCM_ERR_HIP;
        }
    }
    pe25d_join_tracers(m, s);
    const int set = which == 1 ? 2 : m->cur_i;
    TracerStatsArgs a{};
    a.tr = m->tr.n > 0 ? tr_field(m, which, 0) : nullptr;
    a.tstride = tr_stride(m);
    a.q = state_field(m, set, GCM_Q);
    a.p = state_field(m, set, GCM_P);
    a.dsig = m->tr.stats_dev;
    a.out = m->tr.stats_dev + m->L;
    a.part = a.out + n_out;
    a.ntr = m->tr.n; a.nf = nf; a.W = m->W; a.H = m->H; a.L = m->L;
    launch_tracer_stats(a, m->f32, s);
    double rec[GCM_TRACER_STATS_WORDS * (GCM_MAX_TRACERS + 1)];
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(rec, a.out, sizeof(double) * GCM_TRACER_STATS_WORDS * nf, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_status(e, "gcm_tracer_stats", err);
    std::copy(rec, rec + GCM_TRACER_STATS_WORDS * nf, out);
    return GCM_OK;
}

// ---------------------------------------------------------------- a band's ghost-row message
// tr_ghost rows x L levels of every tracer a side (gcm_set_band_tracers, gcm_set_band_tracer_rows)
size_t tracer_halo_bytes(const Pe25d *m) { return m->wrap ? 0 : elem_size(m) * (size_t)m->tr.n * tr_ghost(m) * m->L * m->W; }

// one segment per tracer: those of state set `set` (star with the predicted state, else current)
void tracer_halo_segments(Pe25d *m, bool pack, int side, int set, double **msg, SegCopy *c) {
    if (m->wrap) return;
    const size_t words = (size_t)m->L * m->W * elem_size(m) / 8;
    for (int f = 0; f < m->tr.n; ++f) halo_segment(c, pack, side, tr_field(m, set == 2 ? 1 : 0, f), m->H, tr_ghost(m), words, msg);
}

}  // namespace gcm

// GCM_PE25D: the handle's life cycle and data movement -- pe25d_create (with the one reader of the GCM_PE_* switches)
// and pe25d_destroy, the buffers and tables, the streams that run beside the caller's, set / get with the layout
// transposes, a band's halo buffers and the segments of its ghost-row message, and what the phases behind the dynamics
// share (their column sums, the level table, what a launch of theirs invalidates).  The stage that runs on all this:
// pe25d_kernels.hip; the handle itself: pe25d_host.h.
#include "pe25d_host.h"
#include "pe25d_phase_geometry.h"

namespace gcm {

// ---------------------------------------------------------------- layout transposes
// host layout [k][j][i] (rows of THIS band only, always float64) <-> device [j][k][i] in the
// handle's real type
template <typename T>
__global__ void pe_to_device_kernel(T *dst, const double *src, int W, int H, int L) {
    const long n = (long)W * H * L;
    for (long x = (long)blockIdx.x * blockDim.x + threadIdx.x; x < n; x += (long)gridDim.x * blockDim.x) {
        const int i = x % W;
        const long r = x / W;
        const int k = r % L, j = r / L;
        dst[x] = (T)src[((long)k * H + j) * W + i];
    }
}
template <typename T>
__global__ void pe_to_host_kernel(double *dst, const T *src, int W, int H, int L) {
    const long n = (long)W * H * L;
    for (long x = (long)blockIdx.x * blockDim.x + threadIdx.x; x < n; x += (long)gridDim.x * blockDim.x) {
        const int i = x % W;
        const long r = x / W;
        const int k = r % L, j = r / L;
        dst[((long)k * H + j) * W + i] = (double)src[x];
    }
}

static_assert(sizeof(SegCopy::n) / sizeof(long) >= 2 * (GCM_NFIELDS + 1 + GCM_MAX_TRACERS),
              "SegCopy holds one message per side: 5 fields, the ground temperature and every tracer");

// host float64 table -> device table in T
template <typename T>
static bool upload_as(Pe25d *m, T **dst, const double *src, size_t count) {
    std::vector<T> tmp(count);
    for (size_t i = 0; i < count; ++i) tmp[i] = (T)src[i];
    return dev_upload<T>(m, dst, tmp.data(), count);
}

template <typename T>
static const char *alloc_all(Pe25d *m, const gcm_config &cfg) {
    PeBufs<T> &B = bufs<T>(m);
    const int W = m->W, L = m->L, Hg = m->Hg;
    const size_t n2 = rows_alloc(m) * W, n3 = n2 * L;
    for (int s = 0; s < 3; ++s)
        for (int f = 0; f < GCM_NFIELDS; ++f) {
            T *d = nullptr;
            if (!dev_upload<T>(m, &d, nullptr, f == GCM_P ? n2 : n3)) return "state";
            B.st[s][f] = d + (size_t)kGhost * W * (f == GCM_P ? 1 : L);
        }
    T **inter3[] = {&B.spu, &B.phi, &B.pgfu};
    for (T **pp : inter3) {
        T *d = nullptr;
        if (!dev_upload<T>(m, &d, nullptr, n3)) return "intermediate";
        *pp = d + (size_t)kGhost * W * L;
    }
    T **inter2[] = {&B.pit, &B.pn};
    for (T **pp : inter2) {
        T *d = nullptr;
        if (!dev_upload<T>(m, &d, nullptr, n2)) return "intermediate";
        *pp = d + (size_t)kGhost * W;
    }
    for (int st = 0; st < 3; ++st)
        for (int f = 0; f < 2; ++f) {
            T *d = nullptr;
            if (!dev_upload<T>(m, &d, nullptr, n2)) return "intermediate";
            B.cs[st][f] = d + (size_t)kGhost * W;
        }
    {
        T *d = nullptr;
        if (!dev_upload<T>(m, &d, nullptr, n2 * (kMaxSeg - 1))) return "intermediate";
        B.part = d + (size_t)kGhost * W;
    }
    // tables
    std::vector<double> idj(Hg), idh(Hg), ids(L);
    for (int j = 0; j < Hg; ++j) {
        idj[j] = 1.0 / cfg.dx_j[j];
        idh[j] = 1.0 / cfg.dx_h[j];
    }
    for (int k = 0; k < L; ++k) ids[k] = 1.0 / cfg.dsig[k];
    if (!upload_as<T>(m, &B.inv_dxj, idj.data(), Hg) || !upload_as<T>(m, &B.inv_dxh, idh.data(), Hg) ||
        !upload_as<T>(m, &B.sig, cfg.sig, L) || !upload_as<T>(m, &B.dsig, cfg.dsig, L) ||
        !upload_as<T>(m, &B.inv_dsig, ids.data(), L) || !upload_as<T>(m, &B.sigb, cfg.sigb, L) ||
        !upload_as<T>(m, &B.sigt, cfg.sigt, L))
        return "tables";
    if (cfg.heightmap && !upload_as<T>(m, &B.heightmap, cfg.heightmap, (size_t)Hg * W)) return "heightmap";
    if (cfg.cor_u && (!upload_as<T>(m, &B.cor_u, cfg.cor_u, Hg) || !upload_as<T>(m, &B.cor_v, cfg.cor_v, Hg)))
        return "coriolis tables";
    if (W > 1) {
        // filter multiplier, low_pass.py:61-72, same expression order as the reference
        const int nh = W / 2 + 1;
        std::vector<double> S((size_t)Hg * nh);
        for (int j = 0; j < Hg; ++j) {
            const double drat = cfg.dy / cfg.dx_j[j];
            S[(size_t)j * nh] = 1.0;
            for (int n = 1; n < nh; ++n) {
                const double bysn = 1.0 / std::sin(M_PI / W * (double)n);
                const double sm = 1.0 - bysn / drat;
                S[(size_t)j * nh + n] = 1.0 - std::fmax(sm, 0.0);
            }
        }
        if (!upload_as<T>(m, &B.smul, S.data(), S.size())) return "filter multiplier";
        using T2 = typename Vec2<T>::type;
        std::vector<T2> tw(W);
        for (int n = 0; n < W; ++n) {
            const long double ang = -2.0L * 3.14159265358979323846264338327950288L * n / W;
            tw[n].x = (T)cosl(ang);
            tw[n].y = (T)sinl(ang);
        }
        if (!dev_upload<T2>(m, &B.tw, tw.data(), W)) return "twiddles";
    }
    return nullptr;
}

// A second stream that really runs beside `main`.  HIP maps streams onto a few hardware queues
// round-robin; two streams on one queue execute in order, and which streams share depends on how
// many were created before (with RCCL initialised in the process the library's second stream
// landed on the compute stream's queue: every kernel of a stage serialised; the comm stream on it
// made the exchange wait for the interior rows).  So: create a few candidates, run a 100 us spin
// kernel on `main` (and `other`) and on the candidate at once, and keep the first candidate for
// which they all overlapped.
__global__ void spin_kernel(long long ticks) {
    const long long t0 = wall_clock64();          // 100 MHz
    while (wall_clock64() - t0 < ticks) {
    }
}

// a kernel that does nothing for `us` microseconds (the loopback exchange's stand-in for a transfer time)
void launch_spin(hipStream_t s, double us) {
    if (us > 0) hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, s, (long long)(us * 100.0));
}

hipStream_t concurrent_stream(hipStream_t main, hipStream_t other) {
    constexpr int kCandidates = 6;
    constexpr long long kSpinTicks = 10000;       // 100 us
    hipStream_t cand[kCandidates] = {};
    hipEvent_t e0 = nullptr, ea = nullptr, eb = nullptr, ec = nullptr;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&ea) != hipSuccess || hipEventCreate(&eb) != hipSuccess ||
        hipEventCreate(&ec) != hipSuccess)
        return nullptr;
    int pick = -1, made = 0;
    const char *vb = getenv("GCM_VERBOSE");
    const bool verbose = vb && vb[0] == '1';
    for (int c = 0; c < kCandidates && pick < 0; ++c) {
        if (hipStreamCreateWithFlags(&cand[c], hipStreamNonBlocking) != hipSuccess) break;
        ++made;
        float best = 1e30f;
        for (int rep = 0; rep < 3; ++rep) {
            (void)hipStreamSynchronize(main);
            if (other) (void)hipStreamSynchronize(other);
            (void)hipStreamSynchronize(cand[c]);
            (void)hipEventRecord(e0, main);
            hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, main, kSpinTicks);
            if (other) hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, other, kSpinTicks);
            hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, cand[c], kSpinTicks);
            (void)hipEventRecord(ea, main);
            if (other) (void)hipEventRecord(ec, other);
            (void)hipEventRecord(eb, cand[c]);
            (void)hipStreamSynchronize(main);
            if (other) (void)hipStreamSynchronize(other);
            (void)hipStreamSynchronize(cand[c]);
            float ta = 0.f, tb = 0.f, tc = 0.f;
            (void)hipEventElapsedTime(&ta, e0, ea);
            (void)hipEventElapsedTime(&tb, e0, eb);
            if (other) (void)hipEventElapsedTime(&tc, e0, ec);
            best = std::min(best, std::max(ta, std::max(tb, tc)));
        }
        if (verbose) fprintf(stderr, "gcmcore: stream candidate %d: the 100 us spins took %.1f us\n", c, best * 1e3f);
        if (best < 0.16f) pick = c;               // all spins inside 160 us: they overlapped
    }
    if (pick < 0 && made > 0) pick = 0;           // none overlaps: still correct, only serialised
    for (int c = 0; c < made; ++c)
        if (c != pick) (void)hipStreamDestroy(cand[c]);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(ea);
    (void)hipEventDestroy(eb);
    (void)hipEventDestroy(ec);
    if (verbose) fprintf(stderr, "gcmcore: picked stream candidate %d of %d\n", pick, made);
    return pick >= 0 ? cand[pick] : nullptr;
}

hipStream_t pe25d_aux_stream(const Pe25d *m) { return m->aux; }
// something chain B reads was queued on the caller's stream by somebody else (ghost rows unpacked there, the ground
// temperature uploaded): the next stage's chain B follows that stream's position, not just the last K4
void pe25d_fork_invalidate(Pe25d *m) { m->k4_fork_valid = false; }
void pe25d_set_edges_first(Pe25d *m, bool on) { m->edges_first = on; }
int pe25d_new_state_set(const Pe25d *m) { return (m->pack_set >= 0 && m->pack_set != 2) ? m->pack_set : m->cur_i; }

// ---------------------------------------------------------------- what the phases behind the dynamics share
// Behind a launch that changes rows of state set `set` in place on the caller's stream: theta (and q) always, u and v
// too where wrote_uv (the Held-Suarez forcing and the boundary layer; the moist physics and the convective adjustment write theta and q and
// read p, theta and q).  What the handle remembers about that state is corrected here, once for every such phase:
//  * the column sums K4 left for this state (sum_k dsig u, sum_k dsig v: pit of the next stage) belong to the winds as
//    they were.  They stay valid where u and v are not touched, and for the same reason the wait for the third stream's
//    column sums of the edge rows (which read u and v) is not needed.  wrote_uv: they are no longer valid, and the next
//    stage sums every row again (prep_rows, the path of a freshly set state) -- on a band too, where
//    pe25d_prep_ghost_rows then leaves the ghost rows' sums to that launch.  A single domain and a band so form them by
//    the same kernel in the same order: the same bits;
//  * the fork at the last K4 stays behind a launch that leaves u and v alone, as behind the in-place radiation: what the
//    next stage queues on the second and third stream ahead of its wait for this stream (ev_join, behind K3) -- the ghost
//    rows' column sums and anchors, K1 and pit, the edge rows' partial sums, the tracers -- reads u, v, p, the
//    intermediates and ghost-row theta, never own-row theta or q, and writes none of p, theta, q of this set; the edge
//    rows' K4, which reads them, waits for ev_join.  The exception is a band whose ghost rows the launch takes with the
//    own rows on this stream (gcm_moist_step, gcm_convect_step, the host-driven exchange): the ghost rows' anchors on the
//    second stream read their theta, so chain B must follow this stream's position.  wrote_uv: chain B (K1, the column
//    sums) reads u and v, so it may never fork at the last K4's stop event: it follows this stream's position (ev_fork,
//    recorded behind the launch), and so does everything that waits for that fork;
//  * the ghost rows' geopotential anchors were formed from theta as it was, unless the caller forces the ghost rows
//    itself ahead of them (keep_ghosts: gcm_band_run);
//  * the parity tap's stage state is gone: theta changed.
void pe25d_phase_wrote(Pe25d *m, int set, bool keep_ghosts, bool wrote_uv) {
    if (wrote_uv) m->cs_valid[set] = false;
    if (wrote_uv || !(keep_ghosts || m->wrap)) m->k4_fork_valid = false;
    if (!keep_ghosts) m->ghost_ready = -1;
    m->last_stage_set = -1;                                // gcm_get_intermediate: theta changed
}

const double *pe25d_level_table(Pe25d *m, const char *who, std::string *err) {
    if (m->lev_tab) return m->lev_tab;
    std::vector<double> t(m->sig_host);
    t.insert(t.end(), m->dsig_host.begin(), m->dsig_host.end());
    if (!dev_upload<double>(m, &m->lev_tab, t.data(), t.size())) *err = std::string("hip: ") + who + " table upload failed";
    return m->lev_tab;
}

static PeColumnSums &sums_of(Pe25d *m, PeSums of) {
    return of == kSumsMoist ? m->moist.sums : of == kSumsBoundary ? m->boundary.sums : of == kSumsBettsMiller ? m->betts_miller.sums : m->convect.sums;
}
static size_t sums_words(const Pe25d *m) { return (size_t)m->H * m->W; }
static int sums_zero(Pe25d *m, PeColumnSums &z, const std::string &fn, hipStream_t s, std::string *err) {
    if (int rc = hip_rc(hipMemsetAsync(z.acc, 0, sizeof(double) * 2 * sums_words(m), s), fn.c_str(), err)) return rc;
    z.seconds = 0.0;
    z.n = 0;
    return GCM_OK;
}
// fn: the entry point's name, "gcm_" + pre + <name> + post
static int sums_registered(Pe25d *m, PeSums of, const char *pre, const char *post, std::string *fn, std::string *err) {
    const PeSumsWords &w = kPeSumsWords[of];
    *fn = std::string("gcm_") + pre + w.name + post;
    if (sums_of(m, of).acc) return GCM_OK;
    *err = *fn + ": no " + w.what + " registered (gcm_set_" + w.name + ")";
    return GCM_ERR_STATE;
}

bool pe25d_sums_on(const Pe25d *m, PeSums of) { return sums_of(const_cast<Pe25d *>(m), of).acc != nullptr; }

// gcm_set_<phase>: on -- the accumulators in place and zero; off -- freed
int pe25d_sums_set(Pe25d *m, PeSums of, bool on, hipStream_t s, std::string *err) {
    PeColumnSums &z = sums_of(m, of);
    const std::string fn = std::string("gcm_set_") + kPeSumsWords[of].name;
    if (!on) {
        if (!z.acc) return GCM_OK;
        // (a launch may still be adding to the sums)
        if (int rc = hip_rc(hipStreamSynchronize(s), fn.c_str(), err)) return rc;
        m->allocs.erase(std::remove(m->allocs.begin(), m->allocs.end(), (void *)z.acc), m->allocs.end());
        (void)hipFree(z.acc);
        z = PeColumnSums{};
        return GCM_OK;
    }
    if (z.acc) return sums_zero(m, z, fn, s, err);
    if (!dev_upload<double>(m, &z.acc, nullptr, 2 * sums_words(m))) { *err = "hip: " + fn + " allocation failed"; return GCM_ERR_HIP; }
    z.seconds = 0.0;
    z.n = 0;
    return GCM_OK;
}

int pe25d_sums_reset(Pe25d *m, PeSums of, hipStream_t s, std::string *err) {
    std::string fn;
    if (int rc = sums_registered(m, of, "", "_reset", &fn, err)) return rc;
    return sums_zero(m, sums_of(m, of), fn, s, err);
}

int pe25d_sums_get(Pe25d *m, PeSums of, double *a, double *b, double *seconds, int64_t *nsteps, hipStream_t s, std::string *err) {
    std::string fn;
    if (int rc = sums_registered(m, of, "get_", "", &fn, err)) return rc;
    const PeColumnSums &z = sums_of(m, of);
    const size_t bytes = sizeof(double) * sums_words(m);
    hipError_t e = hipSuccess;
    if (a) e = hipMemcpyAsync(a, z.acc, bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && b) e = hipMemcpyAsync(b, z.acc + sums_words(m), bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (int rc = hip_rc(e, fn.c_str(), err)) return rc;
    if (seconds) *seconds = z.seconds;
    if (nsteps) *nsteps = z.n;
    return GCM_OK;
}

int pe25d_sums_put(Pe25d *m, PeSums of, const double *a, const double *b, double seconds, int64_t nsteps, hipStream_t s, std::string *err) {
    std::string fn;
    if (int rc = sums_registered(m, of, "put_", "", &fn, err)) return rc;
    if (!a || !b || !std::isfinite(seconds) || seconds < 0.0 || nsteps < 0) {
        const PeSumsWords &w = kPeSumsWords[of];
        *err = fn + ": " + w.a + " and " + w.b + " are required, seconds must be finite and >= 0, nsteps >= 0";
        return GCM_ERR_ARG;
    }
    PeColumnSums &z = sums_of(m, of);
    const size_t bytes = sizeof(double) * sums_words(m);
    hipError_t e = hipMemcpyAsync(z.acc, a, bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(z.acc + sums_words(m), b, bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);          // (the caller's arrays are free again when the call returns)
    if (int rc = hip_rc(e, fn.c_str(), err)) return rc;
    z.seconds = seconds;
    z.n = nsteps;
    return GCM_OK;
}

// ---------------------------------------------------------------- what the four sampled diagnostics share
static PeSampler &sampler_of(Pe25d *m, PeSample of) {
    switch (of) {
    case kSamplePlevClimate: return m->plev;
    case kSampleSpectra: return m->spec;
    case kSamplePlevMaps: return m->pmaps;
    default: return m->clim;
    }
}
// the entry point's name, "gcm_" + pre + <name> + post
static std::string sampler_fn(PeSample of, const char *pre, const char *post) {
    return std::string("gcm_") + pre + kPeSamplerWords[of].name + post;
}

int pe25d_sampler_registered(const Pe25d *m, PeSample of, const char *fn, std::string *err) {
    if (sampler_of(const_cast<Pe25d *>(m), of).every > 0) return GCM_OK;
    const PeSamplerWords &w = kPeSamplerWords[of];
    *err = std::string(fn) + ": no " + w.what + " registered (gcm_set_" + w.name + ")";
    return GCM_ERR_STATE;
}

int pe25d_sampler_every(const Pe25d *m, PeSample of) { return sampler_of(const_cast<Pe25d *>(m), of).every; }

bool pe25d_sampler_due(Pe25d *m, PeSample of) {
    PeSampler &z = sampler_of(m, of);
    if (z.every <= 0) return false;
    return ++z.steps % z.every == 0;
}

int pe25d_sampler_reset(Pe25d *m, PeSample of, hipStream_t s, std::string *err) {
    const std::string fn = sampler_fn(of, "", "_reset");
    if (int rc = pe25d_sampler_registered(m, of, fn.c_str(), err)) return rc;
    PeSampler &z = sampler_of(m, of);
    if (int rc = hip_rc(hipMemsetAsync(z.buf + z.head, 0, sizeof(double) * (z.words[0] + z.words[1]), s), fn.c_str(), err)) return rc;
    z.n = 0;
    return GCM_OK;
}

int pe25d_sampler_get(Pe25d *m, PeSample of, double *a, double *b, int64_t *nsamples, hipStream_t s, std::string *err) {
    const std::string fn = sampler_fn(of, "get_", "");
    if (int rc = pe25d_sampler_registered(m, of, fn.c_str(), err)) return rc;
    const PeSampler &z = sampler_of(m, of);
    const double *sums = z.buf + z.head;
    hipError_t e = hipSuccess;
    if (a) e = hipMemcpyAsync(a, sums, sizeof(double) * z.words[0], hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && b) e = hipMemcpyAsync(b, sums + z.words[0], sizeof(double) * z.words[1], hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (int rc = hip_rc(e, fn.c_str(), err)) return rc;
    if (nsamples) *nsamples = z.n;
    return GCM_OK;
}

int pe25d_sampler_put(Pe25d *m, PeSample of, const double *a, const double *b, int64_t nsamples, hipStream_t s, std::string *err) {
    const std::string fn = sampler_fn(of, "put_", "");
    if (int rc = pe25d_sampler_registered(m, of, fn.c_str(), err)) return rc;
    const PeSamplerWords &w = kPeSamplerWords[of];
    if (!a || (w.b && !b) || nsamples < 0) {
        *err = fn + ": " + w.a + (w.b ? std::string(" and ") + w.b + " are" : std::string(" is")) + " required, nsamples must be >= 0";
        return GCM_ERR_ARG;
    }
    PeSampler &z = sampler_of(m, of);
    double *sums = z.buf + z.head;
    hipError_t e = hipMemcpyAsync(sums, a, sizeof(double) * z.words[0], hipMemcpyHostToDevice, s);
    if (e == hipSuccess && w.b) e = hipMemcpyAsync(sums + z.words[0], b, sizeof(double) * z.words[1], hipMemcpyHostToDevice, s);
    const hipError_t es = hipStreamSynchronize(s);             // (also where a copy failed: the caller's arrays are free again when the call returns)
    if (e == hipSuccess) e = es;
    if (int rc = hip_rc(e, fn.c_str(), err)) return rc;
    z.n = nsamples;
    return GCM_OK;
}

void pe25d_sampler_free(Pe25d *m, PeSample of) {
    PeSampler &z = sampler_of(m, of);
    if (z.buf) {
        m->allocs.erase(std::remove(m->allocs.begin(), m->allocs.end(), (void *)z.buf), m->allocs.end());
        (void)hipFree(z.buf);
    }
    z = PeSampler{};
}

// The GCM_PE_* switches, read once per handle at the top of pe25d_create (read_switches) and applied where the handle's
// fields are decided.  Unset = the default.  `num` below is atoi of the value, `c0` its first character.
//   switch                    default                          meaning
//   GCM_PE_LEVEL_SEGMENTS     unset: 1                         K4 marches the column in num level segments, 1 .. min(kMaxSeg, L / 4)
//   GCM_PE_PIT2D              1                                num == 0: pit from the 3-D fields (pe_pit_kernel), not the column sums
//   GCM_PE_UPDATE_ROWS        3 (H <= 400 or fp32), else 7     rows per workgroup of K4: num == 3 -> 3, anything else -> 7
//   GCM_PE_EDGE_SEGMENTS      min(kMaxSeg, L / 6), at least 1  a band: level segments of the edge rows' K4, 1 .. kMaxSeg (1 if L / num < 2)
//   GCM_PE_SINGLE_STREAM      off                              c0 == '1' (diagnostic): one chain, one stream -- no second or third stream
//   GCM_PE_K1_SPLIT           1                                num == 0: K1 of all rows behind the exchange (no third stream)
//   GCM_PE_STOP_EVENTS        1                                num == 0: events recorded behind the kernels, not signalled by them
//   GCM_PE_FILTER_NO_LOOP     off                              set to anything (diagnostic): K1 as one workgroup per level pair
//   GCM_PE_K4_ODDTOP          1                                c0 == '0': K4's whole columns start on an even level
//   GCM_PE_RAD_GENERIC        off                              set to anything (diagnostic): the LDS-parked radiation kernel for every L
struct PeSwitch { bool set = false; int num = 0; char c0 = '\0'; };
struct PeSwitches {
    PeSwitch level_segments, pit2d, update_rows, edge_segments, single_stream, k1_split, stop_events, filter_no_loop, k4_oddtop, rad_generic;
};
static PeSwitches read_switches() {
    const auto sw = [](const char *name) {
        PeSwitch v;
        if (const char *e = getenv(name)) { v.set = true; v.num = atoi(e); v.c0 = e[0]; }
        return v;
    };
    PeSwitches v;
    v.level_segments = sw("GCM_PE_LEVEL_SEGMENTS");
    v.pit2d = sw("GCM_PE_PIT2D");
    v.update_rows = sw("GCM_PE_UPDATE_ROWS");
    v.edge_segments = sw("GCM_PE_EDGE_SEGMENTS");
    v.single_stream = sw("GCM_PE_SINGLE_STREAM");
    v.k1_split = sw("GCM_PE_K1_SPLIT");
    v.stop_events = sw("GCM_PE_STOP_EVENTS");
    v.filter_no_loop = sw("GCM_PE_FILTER_NO_LOOP");
    v.k4_oddtop = sw("GCM_PE_K4_ODDTOP");
    v.rad_generic = sw("GCM_PE_RAD_GENERIC");
    return v;
}

Pe25d *pe25d_create(const gcm_config &cfg, hipStream_t main_stream, std::string *err) {
    const PeSwitches env = read_switches();
    if (!cfg.dx_j || !cfg.dx_h || !cfg.sig || !cfg.dsig || !cfg.sigb || !cfg.sigt) {
        *err = "GCM_PE25D: geometry tables (dx_j, dx_h, sig, dsig, sigb, sigt) are required";
        return nullptr;
    }
    if (!(cfg.dy > 0)) { *err = "GCM_PE25D: dy must be > 0"; return nullptr; }
    if (cfg.global_height < cfg.height || cfg.row0 < 0 || cfg.row0 + cfg.height > cfg.global_height) {
        *err = "GCM_PE25D: band rows outside the global grid";
        return nullptr;
    }
    if (cfg.nranks == 1 && cfg.global_height != cfg.height) {
        *err = "GCM_PE25D: nranks == 1 needs height == global_height";
        return nullptr;
    }
    if (cfg.filter && cfg.width > 1 && cfg.width % 2) {
        *err = "GCM_PE25D: the zonal filter needs an even width (low_pass.py:57; numpy irfft)";
        return nullptr;
    }
    if ((cfg.cor_u != nullptr) != (cfg.cor_v != nullptr)) {
        *err = "GCM_PE25D: cor_u and cor_v must be given together";
        return nullptr;
    }
    if (cfg.dtype != GCM_F64 && cfg.dtype != GCM_F32) { *err = "GCM_PE25D: bad dtype"; return nullptr; }
    Pe25d *m = new Pe25d;
    m->cfg = cfg;
    m->W = cfg.width;
    m->H = cfg.height;
    m->L = cfg.layers;
    m->Hg = cfg.global_height;
    m->wrap = cfg.nranks == 1;
    m->f32 = cfg.dtype == GCM_F32;
    m->dsig_host.assign(cfg.dsig, cfg.dsig + cfg.layers);
    m->sig_host.assign(cfg.sig, cfg.sig + cfg.layers);
    m->sigt_host.assign(cfg.sigt, cfg.sigt + cfg.layers);
    m->dxj_host.assign(cfg.dx_j, cfg.dx_j + cfg.global_height);
    m->dxh_host.assign(cfg.dx_h, cfg.dx_h + cfg.global_height);
    const int W = m->W, L = m->L;
    auto bad = [&](const char *what) {
        *err = std::string("hip: GCM_PE25D allocation/upload failed: ") + what;
        pe25d_destroy(m);
        return (Pe25d *)nullptr;
    };
    if (W > 1) make_super_plan(W, &m->cplan);
    if (W > 1 && (!make_plan(W, &m->plan) || (size_t)W * 32 + 8192 > 160 * 1024)) {
        *err = "GCM_PE25D: width not supported by the in-LDS FFT (too many factors or > 4864)";
        pe25d_destroy(m);
        return nullptr;
    }
    // the LDS-parked column kernels (L > 40: pe_geopot_kernel<T, 0>, pe_radiation_kernel<T, 0>) hold one value per level
    // and thread; the radiation park is the largest (fp64 whatever the handle's type): L <= 156
    const auto layers_fit = [](size_t l) {
        return l * kColThreads * sizeof(double) + kExnerTabDoubles * sizeof(double) <= 160 * 1024 &&
               sizeof(double) * l * kRadThreads + 4096 <= 160 * 1024 && upd_lds_bytes<double>(3, (int)l) + 4096 <= 160 * 1024;
    };
    if (!layers_fit((size_t)L)) {
        int lmax = 1;
        while (layers_fit((size_t)lmax + 1)) ++lmax;
        *err = "GCM_PE25D: " + std::to_string(L) + " layers: the column kernels' LDS holds at most " + std::to_string(lmax);
        pe25d_destroy(m);
        return nullptr;
    }
    {
        // K4 keeps 8 waves per CU resident (2 per SIMD), one row x 62 columns each.  A band with less than
        // about a round and a half of them splits the level march, so that the launch is several short
        // rounds instead of one long one (results do not depend on the split).  Measured on 1440 columns
        // x 24 levels: 90 rows best with 2 segments, 180 and more with 1.  Short bands also take the
        // 3-row workgroups (two per CU, out of step with each other: 3-5 % faster up to ~200 rows; the
        // 7-row form reads the halo rows 9/7 instead of 5/3 times and is kept where bytes matter).
        int dev = 0, cus = 256;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
        m->cus = cus;
        const double rounds = (double)stage_k4_col_tiles(W) * m->H / (8.0 * cus);
        long want = (long)std::ceil(1.5 / std::max(rounds, 1e-3));
        // fp32: 153 VGPRs and 34 KB of tiles per 3-row workgroup let THREE of them share a CU (three waves per SIMD; the
        // 7-row form holds one 8-wave workgroup, two waves per SIMD): c4_f32 1.214 -> 1.126 ms per step (round 4, A/B
        // on one box; 5-row groups, 6 waves, place only one workgroup per CU and take 1.44).  fp64 (215 / 231 VGPRs)
        // stays at two waves per SIMD either way: 3-row groups only where the band is short -- up to 360 rows they win
        // (round 4, one box: a 360-row band of C4 1.050 -> 1.008 ms, of the 2880x1440x40 grid 3.461 -> 3.396), at 720
        // rows the 7-row form does (C4 1.874 vs 1.907, the 2880-column grid 6.597 vs 6.627).
        m->upd_rows = stage_k4_rows(m->H, m->f32);            // (the rule: pe25d_stage_geometry.h)
        if (env.level_segments.set) want = env.level_segments.num;
        if (env.pit2d.set) m->pit2d = env.pit2d.num != 0;      // 0: pit from the 3-D fields (pe_pit_kernel)
        if (env.update_rows.set) m->upd_rows = env.update_rows.num == 3 ? 3 : 7;      // rows per workgroup
        const int cap = std::min(kMaxSeg, std::max(1, L / 4));
        m->nseg = (int)std::max(1L, std::min((long)cap, want));
        // K4 fills the chip with whole columns (a 90-row band: 2 % slower than in two segments) and then
        // leaves the column sums pit needs: segments only on request
        if (!env.level_segments.set) m->nseg = 1;
        if (!m->wrap && m->nseg == 1 && m->pit2d && m->H > 2 * kGhost) {
            m->nseg_edge = std::min(kMaxSeg, std::max(1, L / 6));
            if (env.edge_segments.set) m->nseg_edge = std::max(1, std::min(kMaxSeg, env.edge_segments.num));
            if (L / m->nseg_edge < 2) m->nseg_edge = 1;
        }
    }
    if (const char *what = m->f32 ? alloc_all<float>(m, cfg) : alloc_all<double>(m, cfg)) return bad(what);
    if (!stage_lds_attributes(m) || !radiation_lds_attribute(m)) return bad("dynamic LDS size");
    if (!dev_upload<double>(m, &m->stage3, nullptr, (size_t)m->H * W * L)) return bad("staging");
    double tab[kExnerTabDoubles];
    build_exner_table(tab);
    if (!dev_upload(m, &m->exner_tab, tab, kExnerTabDoubles)) return bad("exner table");
    {
        // ground temperature (column physics), with a band's ghost rows: they travel with every ghost-row message
        double *d = nullptr;
        if (!dev_upload<double>(m, &d, nullptr, rows_alloc(m) * (size_t)W)) return bad("ground temperature");
        m->gt = d + (size_t)kGhost * W;
    }
    // a plain stream: a high-priority one finished the edge rows earlier, but in some processes
    // (depending on how many streams existed before) the whole step then ran at half speed
    if (!(env.single_stream.set && env.single_stream.c0 == '1')) {      // (diagnostic: one chain, one stream)
        m->aux = concurrent_stream(main_stream, nullptr);
        if (!m->aux) return bad("second stream");
        if (env.k1_split.set) m->k1_split = env.k1_split.num != 0;
        if (!m->wrap && m->k1_split) {
            m->aux2 = concurrent_stream(main_stream, m->aux);
            if (!m->aux2) return bad("third stream");
        }
    }
    if (env.stop_events.set) m->stop_events = env.stop_events.num != 0;
    m->filter_no_loop = env.filter_no_loop.set;
    if (env.k4_oddtop.set) m->k4_oddtop = env.k4_oddtop.c0 != '0';
    m->rad_generic = env.rad_generic.set;
    if (hipEventCreateWithFlags(&m->ev_pre_edge, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&m->ev_k4, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&m->ev_cs, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&m->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&m->ev_a, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&m->ev_edges, hipEventDisableTiming) != hipSuccess)
        return bad("events");
    return m;
}

void pe25d_destroy(Pe25d *m) {
    if (!m) return;
    if (m->ev_fork) (void)hipEventDestroy(m->ev_fork);
    if (m->ev_join) (void)hipEventDestroy(m->ev_join);
    if (m->ev_a) (void)hipEventDestroy(m->ev_a);
    if (m->ev_edges) (void)hipEventDestroy(m->ev_edges);
    if (m->ev_cs) (void)hipEventDestroy(m->ev_cs);
    if (m->ev_k4) (void)hipEventDestroy(m->ev_k4);
    if (m->ev_pre_edge) (void)hipEventDestroy(m->ev_pre_edge);
    if (m->aux2) {
        (void)hipStreamSynchronize(m->aux2);
        (void)hipStreamDestroy(m->aux2);
    }
    if (m->aux) {
        (void)hipStreamSynchronize(m->aux);      // (a band's last exchange may still be unpacking)
        (void)hipStreamDestroy(m->aux);
    }
    for (void *p : m->allocs) (void)hipFree(p);
    tracers_destroy(m);
    delete m;
}

// State transfers run on the handle's stream `s` and synchronise only that stream: other handles
// and streams of the process are not stalled.  The float64 staging buffer is reused field by field,
// which the stream order makes safe.
hipError_t field_to_device(Pe25d *m, void *dev_field, const double *host, int levels, hipStream_t s) {
    const hipError_t e = hipMemcpyAsync(m->stage3, host, sizeof(double) * (size_t)m->H * m->W * levels, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    if (m->f32) hipLaunchKernelGGL(pe_to_device_kernel<float>, dim3(1024), dim3(256), 0, s, (float *)dev_field, m->stage3, m->W, m->H, levels);
    else hipLaunchKernelGGL(pe_to_device_kernel<double>, dim3(1024), dim3(256), 0, s, (double *)dev_field, m->stage3, m->W, m->H, levels);
    return hipSuccess;
}
hipError_t field_to_host(Pe25d *m, double *host, const void *dev_field, int levels, hipStream_t s) {
    if (m->f32) hipLaunchKernelGGL(pe_to_host_kernel<float>, dim3(1024), dim3(256), 0, s, m->stage3, (const float *)dev_field, m->W, m->H, levels);
    else hipLaunchKernelGGL(pe_to_host_kernel<double>, dim3(1024), dim3(256), 0, s, m->stage3, (const double *)dev_field, m->W, m->H, levels);
    return hipMemcpyAsync(host, m->stage3, sizeof(double) * (size_t)m->H * m->W * levels, hipMemcpyDeviceToHost, s);
}

static int xfer(Pe25d *m, int set, bool to_dev, const double *const in[GCM_NFIELDS],
                double *const out[GCM_NFIELDS], hipStream_t s, std::string *err) {
    hipError_t e = hipSuccess;
    for (int f = 0; f < GCM_NFIELDS && e == hipSuccess; ++f) {
        if (!(to_dev ? (const void *)in[f] : (const void *)out[f])) continue;
        const int L = f == GCM_P ? 1 : m->L;
        e = to_dev ? field_to_device(m, state_field(m, set, f), in[f], L, s) : field_to_host(m, out[f], state_field(m, set, f), L, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        *err = std::string("pe25d state transfer: ") + hipGetErrorString(e);
        return GCM_ERR_HIP;
    }
    return GCM_OK;
}

int pe25d_set(Pe25d *m, bool star, const double *p, const double *u, const double *v,
              const double *t, const double *q, hipStream_t s, std::string *err) {
    const double *in[GCM_NFIELDS] = {p, u, v, t, q};
    int rc = xfer(m, star ? 2 : m->cur_i, true, in, nullptr, s, err);
    if (u || v) m->cs_valid[star ? 2 : m->cur_i] = false;
    m->ghost_ready = -1;
    if (u || v) m->edge_cs_set = -1;
    m->k4_fork_valid = false;                    // the transposes on the caller's stream: the second stream follows them
    m->last_stage_set = -1;                      // gcm_get_intermediate: the stage state the anchors belong to is gone
    if (rc == GCM_OK) m->star_valid = star;
    return rc;
}

int pe25d_get(Pe25d *m, bool star, double *p, double *u, double *v, double *t, double *q,
              hipStream_t s, std::string *err) {
    if (star && !m->star_valid) {
        *err = "get_star: no predicted state yet";
        return GCM_ERR_STATE;
    }
    double *out[GCM_NFIELDS] = {p, u, v, t, q};
    return xfer(m, star ? 2 : m->cur_i, false, nullptr, out, s, err);
}

int pe25d_set_halo_buffers(Pe25d *m, void *north, void *south, hipStream_t s, std::string *err) {
    if (m->wrap) {
        *err = "set_halo_buffers: handle is not a latitude band";
        return GCM_ERR_STATE;
    }
    if ((north == nullptr) != (south == nullptr)) {
        *err = "set_halo_buffers: give both buffers, or neither to unregister";
        return GCM_ERR_ARG;
    }
    (void)hipStreamSynchronize(s);
    if (m->aux) (void)hipStreamSynchronize(m->aux);
    if (m->aux2) (void)hipStreamSynchronize(m->aux2);
    m->send_buf[0] = north;
    m->send_buf[1] = south;
    m->edges_pending = false;
    if (north) m->halo_fixed = true;             // (gcm_set_band_tracers: the message format is in use from now on)
    return GCM_OK;
}

// ghost rows: [p: 2 rows][u,v,t,q: 2 rows x L levels]; contiguous in the device layout.
// Which state is exchanged follows the step phase: the predicted state once it exists.
size_t pe25d_halo_bytes(const Pe25d *m) {
    // (+ the ground temperature's two rows, float64 for either storage type: gcm_set_physics; + a band's tracers)
    return elem_size(m) * (size_t)kGhost * m->W * (1 + 4 * (size_t)m->L) + sizeof(double) * (size_t)kGhost * m->W + tracer_halo_bytes(m);
}

// appends the copies of one side to *c (the caller launches them: one side or both in one launch)
int pe25d_halo_segments(Pe25d *m, bool pack, int side, void *dev_buf, SegCopy *c, std::string *err) {
    if (m->f32 && (m->W % 2)) {
        *err = "pe25d halo: fp32 bands need an even width";
        return GCM_ERR_UNSUPPORTED;
    }
    // unpack: ghosts of the predicted state once it exists, else of the current state;
    // pack: the same, unless a step_phase call named the set whose edge rows were just produced
    int set = m->star_valid ? 2 : m->cur_i;
    if (pack && m->pack_set >= 0) set = m->pack_set;
    if (!pack && m->pack_set >= 0 && m->pack_set != 2) set = m->pack_set;   // new-state ghosts arrive before the swap
    if (!pack) m->last_unpack_set = set;
    double *msg = (double *)dev_buf;
    for (int f = 0; f < GCM_NFIELDS; ++f)
        halo_segment(c, pack, side, state_field(m, set, f), m->H, kGhost, (size_t)m->W * (f == GCM_P ? 1 : m->L) * elem_size(m) / 8, &msg);
    // the ground temperature: one array for all state sets, advanced by the column physics only.  A band's
    // ghost rows of it are radiated locally (pe25d_solar_rows), so what a message carries equals what the
    // ghost rows hold already -- except in the first exchange after gcm_set_ground, which is what it is for.
    halo_segment(c, pack, side, m->gt, m->H, kGhost, (size_t)m->W, &msg);
    tracer_halo_segments(m, pack, side, set, &msg, c);
    return GCM_OK;
}

// ---------------------------------------------------------------- the phases' launch geometry (gcm_pe25d_phase_plan)
int pe25d_phase_plan(const Pe25d *m, int phase, int rows, bool accumulate, int *out, int nout) {
    return pe25d_phase_geometry(phase, m->W, rows < 0 ? m->H : rows, m->L, m->cus, (int)elem_size(m), accumulate, out, nout);
}

}  // namespace gcm

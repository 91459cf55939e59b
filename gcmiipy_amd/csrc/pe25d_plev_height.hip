// GCM_PE25D, geopotential height on pressure levels and time-mean maps (gcm_plev_height_columns, gcm_plev_height,
// gcm_set_plev_maps and its companions): every column's mid-level geopotential is formed as the model forms it and
// continued inside the layer that brackets each target pressure; the map call returns Z as it is, the sample adds Z,
// the pressure-level quantities of pe25d_plev.h and their products to float64 sums per (target, cell) that live in the
// handle -- nothing is reduced along longitude.  The contract and the word table: include/gcmcore.h; the rule as code:
// pe25d_plev_height.h, shared with the host build.
//
//   per column (float64, the storage type widened exactly, every operation rounded on its own):
//     Z of a valid target: plev_height_march.  In the same bracket, by pe25d_plev.h's linear-in-p routines and formed per
//     level exactly as pe25d_plev.hip forms them -- the same bits gcm_plev_fields returns:
//     T = theta Pi;  uc = 0.5 (u[i] + u[i - 1]), i periodic;  vc = 0.5 (v[j] + v[j - 1]);  q
//     row -1: row H - 1 on a single domain, a band's first north ghost row of v
//
// Contraction is off for the whole file (the Makefile builds it with -ffp-contract=fast-honor-pragmas).
//
// One kernel, two instantiations per real type (the map call, the sample): grid (256-column blocks, rows), one lane per
// column, no barrier behind the table's.  The map call and the sample run the same march (plev_height_march), so a
// column's Z is the same bits in both.
//
// How the column is held: it is not.  phi[0] is a sum over every level, so the lane reads theta of the whole column
// once for that sum and a second time, from the bottom up to the bracket of its last valid target, to carry phi upward;
// the second read is served by L2, where the workgroup's 256 x L values (48 KB at L = 24 in fp64) still are.  The
// alternative, pe_geopot_kernel's -- stp of every level in registers for L <= 24 and L <= 40, parked in LDS above --
// would save that second read and the second evaluation of Pi at the price of three instantiations per real type and
// call, 24 to 40 more float64 registers a lane, and a launcher that picks among them.  It was not taken because most
// of the sample's bytes are elsewhere: per column and sample it reads and writes 2 x 8 x (13 N + 2) bytes of sums, 656
// bytes at three targets, against 192 bytes of theta at L = 24, and the sums do not fit any cache between two samples;
// and because the sample's registers are already what limits its waves (profiles/plev_maps/README.md has the bytes,
// the registers and the measured times).  One path also means that every L runs the code every test runs.  theta is
// requested CHUNK levels at a time (plev_height_chunk<T>(), by real type as measured).
//
// The sums' layout is [word][n][j][i]: a wave's read-modify-write of a word is 64 consecutive doubles.  One writer per
// accumulator word and launch -- the lane that owns the column --, no atomics, no cross-lane reduction; an invalid
// column adds nothing and touches nothing.  u, v and q are read in a target's bracket only.
#pragma clang fp contract(off)
#include "pe25d_host.h"

#include "pe25d_plev_height.h"

namespace gcm {

constexpr int kPhLdsDoubles = kExnerTabDoubles + GCM_PLEV_MAX;   // the Exner table, then Pi of the targets

// level k of column i of row j (row -1: jm): uc, vc, q
struct PlevHeightCell { double uc, vc, q; };
template <typename T>
__device__ __forceinline__ PlevHeightCell plev_height_cell(const PlevHeightArgs &a, int j, int jm, int k, int i) {
    const long r = ((long)j * a.L + k) * a.W, rn = ((long)jm * a.L + k) * a.W;
    const T xu = ((const T *)a.u)[r + i], xw = ((const T *)a.u)[r + (i == 0 ? a.W - 1 : i - 1)];
    const T xv = ((const T *)a.v)[r + i], xn = ((const T *)a.v)[rn + i];
    const T xq = ((const T *)a.q)[r + i];
    PlevHeightCell c;
    c.uc = 0.5 * ((double)xu + (double)xw);
    c.vc = 0.5 * ((double)xv + (double)xn);
    c.q = (double)xq;
    return c;
}

// grid (256-column blocks, rows).  SAMPLE: add to the sums; else write Z, or `fill`, and the mask
template <typename T, bool SAMPLE>
__global__ __launch_bounds__(kPhThreads) void pe_plev_height_kernel(PlevHeightArgs a) {
    __shared__ double lds[kPhLdsDoubles];
    double *tab = lds, *piP = lds + kExnerTabDoubles;
    for (int n = threadIdx.x; n < kExnerTabDoubles; n += kPhThreads) tab[n] = a.exner_tab[n];
    __syncthreads();
    for (int n = threadIdx.x; n < a.N; n += kPhThreads) piP[n] = exner(a.P[n], tab);
    __syncthreads();
    const int W = a.W, L = a.L, H = a.H, N = a.N;
    const int i = (int)(blockIdx.x * kPhThreads + threadIdx.x), j = (int)blockIdx.y;
    if (i >= W) return;
    const int jm = (a.wrap && j == 0) ? H - 1 : j - 1;
    const long cell = (long)j * W + i, plane = (long)H * W;
    const double pc = (double)((const T *)a.p)[cell];
    const double hmG = a.hm ? (double)((const T *)a.hm)[(long)(a.row0 + j) * W + i] * kG : 0.0 * kG;
    const T *tc = (const T *)a.t + (long)j * L * W + i;
    auto th = [&](int k) { return (double)tc[(long)k * W]; };
    if (SAMPLE) {
        const double p1 = a.s2[cell], p2 = a.s2[plane + cell];
        a.s2[cell] = p1 + pc;
        a.s2[plane + cell] = p2 + pc * pc;
        auto hit = [&](int n, int k, double Z, double plk, double plk1, double thk, double thk1, double pik, double pik1) {
            const PlevHeightCell lo = plev_height_cell<T>(a, j, jm, k, i), hi = plev_height_cell<T>(a, j, jm, k + 1, i);
            const double w = plev_weight(plk, plk1, a.P[n]);
            const double tt = plev_interp(w, thk * pik, thk1 * pik1);
            const double uc = plev_interp(w, lo.uc, hi.uc), vc = plev_interp(w, lo.vc, hi.vc), q = plev_interp(w, lo.q, hi.q);
            double *s = a.s + (long)n * plane + cell;
            const long word = (long)N * plane;
            const double term[GCM_PLEV_MAP_WORDS] = {1.0, Z, Z * Z, tt, tt * tt, uc, vc, uc * uc, vc * vc, uc * vc, vc * tt, q, vc * q};
            // (the thirteen words are requested before the first is written back: one memory latency a target, where
            // `s[w * word] += term` would wait for every word in turn -- the compiler cannot tell that they do not overlap)
            double was[GCM_PLEV_MAP_WORDS];
#pragma unroll
            for (int w = 0; w < GCM_PLEV_MAP_WORDS; ++w) was[w] = s[w * word];
#pragma unroll
            for (int w = 0; w < GCM_PLEV_MAP_WORDS; ++w) s[w * word] = was[w] + term[w];
        };
        plev_height_march<plev_height_chunk<T>()>(L, N, a.P, piP, pc, a.ptop, a.lev, hmG, tab, th, hit, [](int) {});
    } else {
        auto put = [&](int n, bool ok, double z) {
            a.out[(long)n * plane + cell] = z;
            if (a.valid) a.valid[(long)n * plane + cell] = ok ? 1 : 0;
        };
        plev_height_march<plev_height_chunk<T>()>(L, N, a.P, piP, pc, a.ptop, a.lev, hmG, tab, th,
                          [&](int n, int, double Z, double, double, double, double, double, double) { put(n, true, Z); },
                          [&](int n) { put(n, false, a.fill); });
    }
}

// ---------------------------------------------------------------- the host build (gcm_plev_height_columns)
int plev_height_columns(int ncol, int L, int N, const double *p, const double *theta, const double *hmG, const double *sig,
                        const double *dsig, const double *sigt, double ptop, const double *P, double *out, int *valid, std::string *err) {
    if (!p || !theta || !sig || !dsig || !sigt || !out || !valid || ncol < 0 || L < 2 || !std::isfinite(ptop)) {
        *err = "gcm_plev_height_columns: p, theta, sig, dsig, sigt, out and valid are required, ncol >= 0, L >= 2, ptop finite";
        return GCM_ERR_ARG;
    }
    if (!plev_targets_ok(N, P)) {
        *err = "gcm_plev_height_columns: 1 .. GCM_PLEV_MAX targets, finite, positive and strictly decreasing";
        return GCM_ERR_ARG;
    }
    double tab[kExnerTabDoubles], piP[GCM_PLEV_MAX];
    build_exner_table(tab);
    for (int n = 0; n < N; ++n) piP[n] = exner(P[n], tab);
    std::vector<double> lev(sig, sig + L);
    lev.insert(lev.end(), dsig, dsig + L);
    lev.insert(lev.end(), sigt, sigt + L);
    for (long c = 0; c < ncol; ++c) {
        const double *tc = theta + c * L;
        double *o = out + c * N;
        int *ok = valid + c * N;
        plev_height_march<kPhHostChunk>(L, N, P, piP, p[c], ptop, lev.data(), hmG ? hmG[c] : 0.0 * kG, tab, [&](int k) { return tc[k]; },
                          [&](int n, int, double Z, double, double, double, double, double, double) { o[n] = Z; ok[n] = 1; },
                          [&](int n) { ok[n] = 0; });
    }
    return GCM_OK;
}

// ---------------------------------------------------------------- the handle's side
// layout of the sampler's buf (doubles): P [N] | s [GCM_PLEV_MAP_WORDS][N][H][W] | s2 [GCM_PLEV_MAP_WORDS2][H][W].  every,
// due, reset, get, put and free are the samplers' shared routines (pe25d_sampler_*, pe25d_state.hip), the targets' query
// pe25d_plev_levels (pe25d_plev.hip)

// sig [L], dsig [L], sigt [L] in float64 on the device, uploaded by the first call and kept until the handle goes
static const double *height_table(Pe25d *m, const char *who, std::string *err) {
    if (m->plev_height_tab) return m->plev_height_tab;
    std::vector<double> t(m->sig_host);
    t.insert(t.end(), m->dsig_host.begin(), m->dsig_host.end());
    t.insert(t.end(), m->sigt_host.begin(), m->sigt_host.end());
    if (!dev_upload<double>(m, &m->plev_height_tab, t.data(), t.size())) *err = std::string("hip: ") + who + " table upload failed";
    return m->plev_height_tab;
}

// what the kernel reads of the handle's current state
static PlevHeightArgs height_args(Pe25d *m) {
    const int set = m->cur_i;
    PlevHeightArgs a{};
    a.p = state_field(m, set, GCM_P); a.u = state_field(m, set, GCM_U); a.v = state_field(m, set, GCM_V);
    a.t = state_field(m, set, GCM_T); a.q = state_field(m, set, GCM_Q);
    a.hm = m->f32 ? (const void *)m->f.heightmap : (const void *)m->d.heightmap;
    a.lev = m->plev_height_tab; a.exner_tab = m->exner_tab;
    a.ptop = m->cfg.ptop;
    a.W = m->W; a.H = m->H; a.L = m->L; a.row0 = m->cfg.row0; a.wrap = m->wrap ? 1 : 0;
    return a;
}

template <bool SAMPLE>
static hipError_t height_launch(const Pe25d *m, const PlevHeightArgs &a, hipStream_t s) {
    const dim3 grid((unsigned)plev_height_chunks(a.W), (unsigned)a.H);
    if (m->f32) hipLaunchKernelGGL((pe_plev_height_kernel<float, SAMPLE>), grid, dim3(kPhThreads), 0, s, a);
    else hipLaunchKernelGGL((pe_plev_height_kernel<double, SAMPLE>), grid, dim3(kPhThreads), 0, s, a);
    return hipGetLastError();
}

static int height_checks(Pe25d *m, const char *fn, int N, const double *P, std::string *err) {
    if (!plev_targets_ok(N, P)) {
        *err = std::string(fn) + ": 1 .. GCM_PLEV_MAX = " + std::to_string(GCM_PLEV_MAX) + " targets in Pa, finite, positive and strictly decreasing";
        return GCM_ERR_ARG;
    }
    if (m->L < 2) { *err = std::string(fn) + ": a column of one level has no bracket to continue the height in"; return GCM_ERR_UNSUPPORTED; }
    if (!height_table(m, fn, err)) return GCM_ERR_HIP;
    return GCM_OK;
}

// A second registration always takes a new buffer, as the pressure-level climatology's; the sums are zeroed on the device
int pe25d_set_plev_maps(Pe25d *m, int every, int N, const double *P, hipStream_t s, std::string *err) {
    PePlev &z = m->pmaps;
    if (every < 0) { *err = "gcm_set_plev_maps: every must be >= 0"; return GCM_ERR_ARG; }
    if (every == 0) {
        if (!z.buf) return GCM_OK;
        // (a sample may still be adding to the sums)
        if (int rc = hip_rc(hipStreamSynchronize(s), "gcm_set_plev_maps", err)) return rc;
        pe25d_sampler_free(m, kSamplePlevMaps);
        return GCM_OK;
    }
    if (int rc = height_checks(m, "gcm_set_plev_maps", N, P, err)) return rc;
    // (the targets change with the registration, and a sample in flight reads the ones in place: a new buffer)
    if (z.buf) {
        if (int rc = hip_rc(hipStreamSynchronize(s), "gcm_set_plev_maps", err)) return rc;
        pe25d_sampler_free(m, kSamplePlevMaps);
    }
    // (the sums are (13 N + 2) H W doubles, hundreds of MB on a product grid: zeroed on the device, not uploaded)
    void *d = nullptr;
    const size_t cells = (size_t)m->H * m->W, sums = (size_t)GCM_PLEV_MAP_WORDS * N * cells, sums2 = (size_t)GCM_PLEV_MAP_WORDS2 * cells;
    hipError_t e = hipMalloc(&d, sizeof(double) * ((size_t)N + sums + sums2));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *err = "hip: gcm_set_plev_maps allocation failed";
        return GCM_ERR_HIP;
    }
    e = hipMemcpyAsync(d, P, sizeof(double) * N, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync((double *)d + N, 0, sizeof(double) * (sums + sums2), s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);          // (the caller's targets are free again when the call returns)
    if (e != hipSuccess) {
        (void)hipFree(d);
        return hip_rc(e, "gcm_set_plev_maps", err);
    }
    m->allocs.push_back(d);
    z.buf = (double *)d;
    z.P.assign(P, P + N);
    z.head = (size_t)N;
    z.words[0] = sums;
    z.words[1] = sums2;
    z.every = every;
    z.steps = 0;
    z.n = 0;
    return GCM_OK;
}

int pe25d_plev_maps_plan(const Pe25d *m, int *out, int nout) {
    if (!out || nout < GCM_PLEV_MAP_PLAN_WORDS) return GCM_ERR_ARG;
    const bool on = m->pmaps.every > 0;
    out[0] = plev_height_chunks(m->W);
    out[1] = on ? m->H : 0;
    out[2] = kPhThreads;
    out[3] = (int)(sizeof(double) * kPhLdsDoubles);
    out[4] = on ? (int)m->pmaps.P.size() : 0;
    return GCM_OK;
}

// The launch reads p, u, v, theta and q of the current state set, on a band v's first north ghost row, and tables nobody
// writes (the heightmap, the levels, the targets); the last sample of a step, behind the climatology's, the pressure-level
// climatology's and the spectra's on `s`.  How it is ordered against the stages that follow: pe25d_kernels.h, at the
// samplers' declarations
int pe25d_plev_maps_sample(Pe25d *m, hipStream_t s, std::string *err) {
    if (int rc = pe25d_sampler_registered(m, kSamplePlevMaps, "gcm_plev_maps_sample", err)) return rc;
    PePlev &z = m->pmaps;
    const int N = (int)z.P.size();
    PlevHeightArgs a = height_args(m);
    a.P = z.buf; a.s = z.buf + z.head; a.s2 = a.s + z.words[0]; a.N = N;
    if (int rc = hip_rc(height_launch<true>(m, a, s), "gcm_plev_maps_sample", err)) return rc;
    ++z.n;
    return GCM_OK;
}

// gcm_plev_height: a pure reader of the current state set on `s`, like the sample; it synchronises `s` before it returns,
// so nothing of it is in flight when the next stage is queued.  The device buffers live for the call only
int pe25d_plev_height(Pe25d *m, int N, const double *P, double fill, double *out, int32_t *valid, hipStream_t s, std::string *err) {
    if (!out) { *err = "gcm_plev_height: out is required"; return GCM_ERR_ARG; }
    if (int rc = height_checks(m, "gcm_plev_height", N, P, err)) return rc;
    const size_t cells = (size_t)N * m->H * m->W;
    double *dout = nullptr, *dP = nullptr;
    int32_t *dvalid = nullptr;
    hipError_t e = hipMalloc((void **)&dout, sizeof(double) * cells);
    if (e == hipSuccess) e = hipMalloc((void **)&dP, sizeof(double) * N);
    if (e == hipSuccess && valid) e = hipMalloc((void **)&dvalid, sizeof(int32_t) * cells);
    if (e == hipSuccess) e = hipMemcpyAsync(dP, P, sizeof(double) * N, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        PlevHeightArgs a = height_args(m);
        a.P = dP; a.N = N; a.out = dout; a.valid = dvalid; a.fill = fill;
        e = height_launch<false>(m, a, s);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, sizeof(double) * cells, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && valid) e = hipMemcpyAsync(valid, dvalid, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, s);
    const hipError_t es = hipStreamSynchronize(s);             // (also where an earlier call failed: P may still be on its way)
    if (e == hipSuccess) e = es;
    (void)hipFree(dout); (void)hipFree(dP); (void)hipFree(dvalid);
    return hip_rc(e, "gcm_plev_height", err);
}

}  // namespace gcm

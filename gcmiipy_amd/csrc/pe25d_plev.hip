// GCM_PE25D on pressure levels (gcm_plev_columns, gcm_plev_fields, gcm_set_plev_climate and its companions): every
// column of the current state is interpolated from the model's sigma levels to a fixed list of pressures, linearly in
// pressure, and masked where the pressure lies under the ground or above the top mid-level; the sample reduces the
// result zonally into float64 sums that live in the handle, the maps come back as they are.  The contract, the word
// table and the column rule: include/gcmcore.h; the rule as code: pe25d_plev.h, shared with the host build.
//
//   per cell and level (float64, the storage type widened exactly, every product and sum rounded on its own), exactly
//   as pe25d_climate.hip forms them:
//     pl = sig[k] p + ptop,  T = theta Pi,  Pi = exner(pl)        (the kernels' own Exner routine, gcm_math.h)
//     uc = 0.5 (u[i] + u[i - 1]), i periodic;   vc = 0.5 (v[j] + v[j - 1])
//     row -1: row H - 1 on a single domain (the model's pole-to-pole roll), a band's first north ghost row of v
//   uc, vc, theta, T and q are interpolated; T is formed on the sigma level and then interpolated.
//
// Contraction is off for the whole file (the Makefile builds it with -ffp-contract=fast-honor-pragmas).
//
// The sample: grid (rows, target segments), 256 threads.  A workgroup owns row j and kPlSegTargets consecutive targets.
// Lane t takes the columns i = t, t + 256, ... in that order.  It marches a column's level pressures upward -- sig[k] p
// + ptop, no load -- and reads the two cells of a bracket only where it holds one of the workgroup's targets
// (plev_in_bracket); the upper cell stays in registers for the next bracket.  The target's thirteen terms go onto the
// lane's sums of that target, which start at 0.0 and stay in registers.  A column in which the target is invalid
// adds nothing, which leaves the bits that adding 0.0 would (a sum that starts at +0.0 never becomes -0.0).  Behind the
// last column the 64 lanes of a wave combine by the xor butterfly 32, 16, .. 1, the four waves in wave order through
// LDS, and thread w < 13 adds the row's sum into word w -- the climatology's order (pe25d_climate.hip), a function of W
// alone.  No atomics, one writer per accumulator word and launch; a target's sums do not depend on which segment holds
// it, on H, the band or the number of CUs.
//
// p of a column is one register for the whole march, so the row is not parked in LDS and no row is too wide for the
// launch; LDS holds the Exner table and the waves' sums.  A (j, k) row is one contiguous run and a wave requests 64
// consecutive i of it where the lanes' targets fall into the same bracket, which they do where p varies little along
// the row.  A segment reads p and, per column, between two and twice its targets' levels of u, v, theta and q; all the
// segments together at most (4 L + 1) H W elements each -- see profiles/plev_climate/README.md for what was measured.
//
// The maps: grid (256-column blocks, rows), one lane per column, the same march with a monotone pointer into the
// targets; every entry of the output is written once, the value or `fill`.
#pragma clang fp contract(off)
#include "pe25d_host.h"

#include "pe25d_plev.h"

namespace gcm {

constexpr int kPlRedDoubles = 2 * kPlWaves * GCM_PLEV_WORDS;   // two buffers of the waves' sums: one barrier per target

size_t plev_lds_bytes() { return sizeof(double) * ((size_t)kExnerTabDoubles + kPlRedDoubles); }

// the five quantities of a cell and its pressure
struct PlevCell { double pl, uc, vc, th, tt, q; };

// column i of row j (row -1: jm) at level k; pc: the column's p
template <typename T>
__device__ __forceinline__ PlevCell plev_cell(const PlevArgs &a, int j, int jm, int k, int i, double pc, const double *tab) {
    const long r = ((long)j * a.L + k) * a.W, rn = ((long)jm * a.L + k) * a.W;
    const T xu = ((const T *)a.u)[r + i], xw = ((const T *)a.u)[r + (i == 0 ? a.W - 1 : i - 1)];
    const T xv = ((const T *)a.v)[r + i], xn = ((const T *)a.v)[rn + i];
    const T xt = ((const T *)a.t)[r + i], xq = ((const T *)a.q)[r + i];
    PlevCell c;
    c.pl = a.sig[k] * pc + a.ptop;
    c.th = (double)xt;
    c.tt = c.th * exner(c.pl, tab);
    c.uc = 0.5 * ((double)xu + (double)xw);
    c.vc = 0.5 * ((double)xv + (double)xn);
    c.q = (double)xq;
    return c;
}

// the workgroup's GCM_PLEV_WORDS sums, in thread w < GCM_PLEV_WORDS (word w): the butterfly, then the waves in order.
// `red`: kPlWaves * GCM_PLEV_WORDS doubles nobody else touches until the next barrier but one
__device__ __forceinline__ double plev_block_sum(double (&s)[GCM_PLEV_WORDS], double *red) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int n = 0; n < GCM_PLEV_WORDS; ++n) s[n] = s[n] + __shfl_xor(s[n], d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int n = 0; n < GCM_PLEV_WORDS; ++n) red[(threadIdx.x >> 6) * GCM_PLEV_WORDS + n] = s[n];
    }
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x < GCM_PLEV_WORDS) {
        r = red[threadIdx.x];
        for (int w = 1; w < kPlWaves; ++w) r = r + red[w * GCM_PLEV_WORDS + threadIdx.x];
    }
    return r;
}

// grid (rows, target segments).  Every thread reaches every barrier: the targets a segment holds depend on the
// workgroup alone, lanes beyond W add nothing
template <typename T>
__global__ __launch_bounds__(kPlThreads) void pe_plev_climate_kernel(PlevArgs a) {
    extern __shared__ __align__(16) double pl_lds[];
    double *tab = pl_lds, *red = tab + kExnerTabDoubles;
    for (int n = threadIdx.x; n < kExnerTabDoubles; n += kPlThreads) tab[n] = a.exner_tab[n];
    __syncthreads();
    const int W = a.W, L = a.L, H = a.H, N = a.N;
    const int j = (int)blockIdx.x, n0 = (int)blockIdx.y * kPlSegTargets;
    const int jm = (a.wrap && j == 0) ? H - 1 : j - 1;
    const T *pj = (const T *)a.p + (long)j * W;
    const double sig0 = a.sig[0], sigt = a.sig[L - 1];
    double P[kPlSegTargets], s[kPlSegTargets][GCM_PLEV_WORDS];
#pragma unroll
    for (int m = 0; m < kPlSegTargets; ++m) {
        P[m] = n0 + m < N ? a.P[n0 + m] : nan("");            // (a NaN target is valid nowhere)
#pragma unroll
        for (int w = 0; w < GCM_PLEV_WORDS; ++w) s[m][w] = 0.0;
    }
    for (int i = (int)threadIdx.x; i < W; i += kPlThreads) {
        const double pc = (double)pj[i];
        const double pl0 = sig0 * pc + a.ptop, plt = sigt * pc + a.ptop;
        bool ok[kPlSegTargets], any = false;
#pragma unroll
        for (int m = 0; m < kPlSegTargets; ++m) {
            ok[m] = plev_valid(pl0, plt, P[m]);
            any = any || ok[m];
            if (ok[m]) s[m][0] = s[m][0] + 1.0;
        }
        if (!any) continue;
        // the march computes the levels' pressures only (sig[k] is a scalar: no load); a bracket's two cells are read
        // where one of the workgroup's targets lies in it -- the cell's own pl is the same expression, the same bits
        PlevCell lo{};
        int klo = -1;                                          // the level `lo` holds
        double plk = pl0;
        for (int k = 0; k + 1 < L; ++k) {
            const double plk1 = a.sig[k + 1] * pc + a.ptop;
            bool in[kPlSegTargets], need = false;
#pragma unroll
            for (int m = 0; m < kPlSegTargets; ++m) {
                in[m] = ok[m] && plev_in_bracket(plk, plk1, k + 2 == L, P[m]);
                need = need || in[m];
            }
            plk = plk1;
            if (!need) continue;
            if (klo != k) lo = plev_cell<T>(a, j, jm, k, i, pc, tab);
            const PlevCell hi = plev_cell<T>(a, j, jm, k + 1, i, pc, tab);
            klo = k + 1;
#pragma unroll
            for (int m = 0; m < kPlSegTargets; ++m) {
                if (!in[m]) continue;
                const double w = plev_weight(lo.pl, hi.pl, P[m]);
                const double uc = plev_interp(w, lo.uc, hi.uc), vc = plev_interp(w, lo.vc, hi.vc);
                const double th = plev_interp(w, lo.th, hi.th), tt = plev_interp(w, lo.tt, hi.tt);
                const double q = plev_interp(w, lo.q, hi.q);
                s[m][1] = s[m][1] + uc;
                s[m][2] = s[m][2] + vc;
                s[m][3] = s[m][3] + th;
                s[m][4] = s[m][4] + tt;
                s[m][5] = s[m][5] + q;
                s[m][6] = s[m][6] + uc * uc;
                s[m][7] = s[m][7] + vc * vc;
                s[m][8] = s[m][8] + tt * tt;
                s[m][9] = s[m][9] + uc * vc;
                s[m][10] = s[m][10] + vc * tt;
                s[m][11] = s[m][11] + vc * th;
                s[m][12] = s[m][12] + vc * q;
            }
            lo = hi;
        }
    }
    // (two buffers: the readers of this target's sums are past them before anyone writes this buffer again, which is
    // behind the next target's barrier)
#pragma unroll
    for (int m = 0; m < kPlSegTargets; ++m) {
        if (n0 + m >= N) break;                                // (the same for the whole workgroup)
        const double r = plev_block_sum(s[m], red + (m & 1) * (kPlWaves * GCM_PLEV_WORDS));
        if (threadIdx.x < GCM_PLEV_WORDS) a.s[((long)threadIdx.x * N + n0 + m) * H + j] += r;
    }
}

// grid (256-column blocks, rows): one lane per column, no barrier behind the table's
template <typename T>
__global__ __launch_bounds__(kPlThreads) void pe_plev_fields_kernel(PlevArgs a) {
    __shared__ double tab[kExnerTabDoubles];
    for (int n = threadIdx.x; n < kExnerTabDoubles; n += kPlThreads) tab[n] = a.exner_tab[n];
    __syncthreads();
    const int W = a.W, L = a.L, H = a.H, N = a.N;
    const int i = (int)(blockIdx.x * kPlThreads + threadIdx.x), j = (int)blockIdx.y;
    if (i >= W) return;
    const int jm = (a.wrap && j == 0) ? H - 1 : j - 1;
    const double pc = (double)((const T *)a.p)[(long)j * W + i];
    const double pl0 = a.sig[0] * pc + a.ptop, plt = a.sig[L - 1] * pc + a.ptop;
    const long cell = (long)j * W + i, plane = (long)H * W;
    // entry n of the column: the five values and the mask word
    auto put = [&](int n, bool ok, double uc, double vc, double th, double tt, double q) {
        double *o = a.out + (long)n * plane + cell;
        o[0] = uc; o[(long)N * plane] = vc; o[2L * N * plane] = th; o[3L * N * plane] = tt; o[4L * N * plane] = q;
        if (a.valid) a.valid[(long)n * plane + cell] = ok ? 1 : 0;
    };
    int n = 0;
    // (the targets under the ground; a column with p <= 0 or a NaN p: all of them)
    while (n < N && !plev_valid(pl0, plt, a.P[n]) && !(a.P[n] < plt)) { put(n, false, a.fill, a.fill, a.fill, a.fill, a.fill); ++n; }
    if (n < N && plev_valid(pl0, plt, a.P[n])) {
        PlevCell lo = plev_cell<T>(a, j, jm, 0, i, pc, tab);
        for (int k = 0; k + 1 < L && n < N; ++k) {
            const PlevCell hi = plev_cell<T>(a, j, jm, k + 1, i, pc, tab);
            while (n < N && plev_valid(pl0, plt, a.P[n]) && plev_in_bracket(lo.pl, hi.pl, k + 2 == L, a.P[n])) {
                const double w = plev_weight(lo.pl, hi.pl, a.P[n]);
                put(n, true, plev_interp(w, lo.uc, hi.uc), plev_interp(w, lo.vc, hi.vc), plev_interp(w, lo.th, hi.th),
                    plev_interp(w, lo.tt, hi.tt), plev_interp(w, lo.q, hi.q));
                ++n;
            }
            lo = hi;
        }
    }
    // (the targets above the top mid-level)
    for (; n < N; ++n) put(n, false, a.fill, a.fill, a.fill, a.fill, a.fill);
}

// ---------------------------------------------------------------- the host build (gcm_plev_columns)
int plev_columns(int ncol, int L, int N, const double *pl, const double *x, const double *P, double *out, int *valid, std::string *err) {
    if (!pl || !x || !out || !valid || ncol < 0 || L < 2) {
        *err = "gcm_plev_columns: pl, x, out and valid are required, ncol >= 0, L >= 2";
        return GCM_ERR_ARG;
    }
    if (!plev_targets_ok(N, P)) {
        *err = "gcm_plev_columns: 1 .. GCM_PLEV_MAX targets, finite, positive and strictly decreasing";
        return GCM_ERR_ARG;
    }
    for (long c = 0; c < ncol; ++c) plev_column(L, N, pl + c * L, x + c * L, P, out + c * N, valid + c * N);
    return GCM_OK;
}

// ---------------------------------------------------------------- the handle's side
// layout of the sampler's buf (doubles): P [N] | s [GCM_PLEV_WORDS][N][H].  every, due, reset, get, put and free are the
// samplers' shared routines (pe25d_sampler_*, pe25d_state.hip)

// what both kernels read of the handle's current state
static PlevArgs plev_args(Pe25d *m, const double *sig) {
    const int set = m->cur_i;
    PlevArgs a{};
    a.p = state_field(m, set, GCM_P); a.u = state_field(m, set, GCM_U); a.v = state_field(m, set, GCM_V);
    a.t = state_field(m, set, GCM_T); a.q = state_field(m, set, GCM_Q);
    a.sig = sig; a.exner_tab = m->exner_tab;
    a.ptop = m->cfg.ptop;
    a.W = m->W; a.H = m->H; a.L = m->L; a.wrap = m->wrap ? 1 : 0;
    return a;
}

// A second registration always takes a new buffer: the targets change with it
int pe25d_set_plev_climate(Pe25d *m, int every, int N, const double *P, hipStream_t s, std::string *err) {
    PePlev &z = m->plev;
    if (every < 0) { *err = "gcm_set_plev_climate: every must be >= 0"; return GCM_ERR_ARG; }
    if (every == 0) {
        if (!z.buf) return GCM_OK;
        // (a sample may still be adding to the sums)
        if (int rc = hip_rc(hipStreamSynchronize(s), "gcm_set_plev_climate", err)) return rc;
        pe25d_sampler_free(m, kSamplePlevClimate);
        return GCM_OK;
    }
    if (!plev_targets_ok(N, P)) {
        *err = "gcm_set_plev_climate: 1 .. GCM_PLEV_MAX = " + std::to_string(GCM_PLEV_MAX) + " targets in Pa, finite, positive and strictly decreasing";
        return GCM_ERR_ARG;
    }
    if (m->L < 2) { *err = "gcm_set_plev_climate: a column of one level has no bracket to interpolate in"; return GCM_ERR_UNSUPPORTED; }
    if (!pe25d_level_table(m, "gcm_set_plev_climate", err)) return GCM_ERR_HIP;
    // (the targets change with the registration, and a sample in flight reads the ones in place: a new buffer)
    if (z.buf) {
        if (int rc = hip_rc(hipStreamSynchronize(s), "gcm_set_plev_climate", err)) return rc;
        pe25d_sampler_free(m, kSamplePlevClimate);
    }
    const size_t sums = (size_t)GCM_PLEV_WORDS * N * m->H;
    std::vector<double> init((size_t)N + sums, 0.0);
    std::copy(P, P + N, init.begin());
    if (!dev_upload<double>(m, &z.buf, init.data(), init.size())) {
        // (dev_upload keeps what it allocated in the handle's list: gcm_destroy frees it)
        z = PePlev{};
        *err = "hip: gcm_set_plev_climate allocation failed";
        return GCM_ERR_HIP;
    }
    z.P.assign(P, P + N);
    z.head = (size_t)N;
    z.words[0] = sums;
    z.words[1] = 0;
    z.every = every;
    z.steps = 0;
    z.n = 0;
    return GCM_OK;
}

// gcm_plev_climate_levels, gcm_plev_maps_levels: the targets of a registration that is in place
int pe25d_plev_levels(const Pe25d *m, PeSample of, double *P, int cap) {
    const PePlev &z = of == kSamplePlevMaps ? m->pmaps : m->plev;
    if (P) std::copy(z.P.begin(), z.P.begin() + std::min<size_t>(z.P.size(), (size_t)std::max(cap, 0)), P);
    return (int)z.P.size();
}

int pe25d_plev_climate_plan(const Pe25d *m, int *out, int nout) {
    if (!out || nout < GCM_PLEV_PLAN_WORDS) return GCM_ERR_ARG;
    out[0] = m->H;
    out[1] = m->plev.every > 0 ? plev_nseg((int)m->plev.P.size()) : 0;
    out[2] = kPlSegTargets;
    out[3] = kPlThreads;
    out[4] = (int)plev_lds_bytes();
    out[5] = plev_chunks(m->W);
    return GCM_OK;
}

// The launch reads p, u, v, theta and q of the current state set, and on a band v's first north ghost row; q is a state
// field, not a tracer.  How it is ordered against the stages that follow: pe25d_kernels.h, at the samplers' declarations
int pe25d_plev_climate_sample(Pe25d *m, hipStream_t s, std::string *err) {
    if (int rc = pe25d_sampler_registered(m, kSamplePlevClimate, "gcm_plev_climate_sample", err)) return rc;
    PePlev &z = m->plev;
    const int N = (int)z.P.size();
    PlevArgs a = plev_args(m, m->lev_tab);
    a.P = z.buf; a.s = z.buf + z.head; a.N = N;
    const dim3 grid((unsigned)a.H, (unsigned)plev_nseg(N));
    if (m->f32) hipLaunchKernelGGL(pe_plev_climate_kernel<float>, grid, dim3(kPlThreads), plev_lds_bytes(), s, a);
    else hipLaunchKernelGGL(pe_plev_climate_kernel<double>, grid, dim3(kPlThreads), plev_lds_bytes(), s, a);
    if (int rc = hip_rc(hipGetLastError(), "gcm_plev_climate_sample", err)) return rc;
    ++z.n;
    return GCM_OK;
}

// gcm_plev_fields: a pure reader of the current state set on `s`, like the sample; it synchronises `s` before it returns,
// so nothing of it is in flight when the next stage is queued.  The device buffers live for the call only
int pe25d_plev_fields(Pe25d *m, int N, const double *P, double fill, double *out, int32_t *valid, hipStream_t s, std::string *err) {
    if (!out) { *err = "gcm_plev_fields: out is required"; return GCM_ERR_ARG; }
    if (!plev_targets_ok(N, P)) {
        *err = "gcm_plev_fields: 1 .. GCM_PLEV_MAX = " + std::to_string(GCM_PLEV_MAX) + " targets in Pa, finite, positive and strictly decreasing";
        return GCM_ERR_ARG;
    }
    if (m->L < 2) { *err = "gcm_plev_fields: a column of one level has no bracket to interpolate in"; return GCM_ERR_UNSUPPORTED; }
    if (!pe25d_level_table(m, "gcm_plev_fields", err)) return GCM_ERR_HIP;
    const size_t cells = (size_t)N * m->H * m->W;
    double *dout = nullptr, *dP = nullptr;
    int32_t *dvalid = nullptr;
    hipError_t e = hipMalloc((void **)&dout, sizeof(double) * kPlFieldQ * cells);
    if (e == hipSuccess) e = hipMalloc((void **)&dP, sizeof(double) * N);
    if (e == hipSuccess && valid) e = hipMalloc((void **)&dvalid, sizeof(int32_t) * cells);
    if (e == hipSuccess) e = hipMemcpyAsync(dP, P, sizeof(double) * N, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        PlevArgs a = plev_args(m, m->lev_tab);
        a.P = dP; a.N = N; a.out = dout; a.valid = dvalid; a.fill = fill;
        const dim3 grid((unsigned)plev_chunks(a.W), (unsigned)a.H);
        if (m->f32) hipLaunchKernelGGL(pe_plev_fields_kernel<float>, grid, dim3(kPlThreads), 0, s, a);
        else hipLaunchKernelGGL(pe_plev_fields_kernel<double>, grid, dim3(kPlThreads), 0, s, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, sizeof(double) * kPlFieldQ * cells, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && valid) e = hipMemcpyAsync(valid, dvalid, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, s);
    const hipError_t es = hipStreamSynchronize(s);             // (also where an earlier call failed: P may still be on its way)
    if (e == hipSuccess) e = es;
    (void)hipFree(dout); (void)hipFree(dP); (void)hipFree(dvalid);
    return hip_rc(e, "gcm_plev_fields", err);
}

}  // namespace gcm

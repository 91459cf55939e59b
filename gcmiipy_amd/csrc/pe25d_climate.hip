// GCM_PE25D, the zonal-mean climatology (gcm_set_climate, gcm_climate_sample, gcm_get_climate): one launch per sample
// reads the current state once, forms the zonal sums over i = 0 .. W - 1 of ten moments per (level, row) and two per
// row, and adds them to float64 sums that live in the handle.  The contract and the moment table: include/gcmcore.h.
//
//   per cell (float64, the storage type widened exactly, every product and sum rounded on its own):
//     T = theta Pi,  Pi = exner(sig[k] p + ptop)                  (the kernels' own Exner routine, gcm_math.h)
//     uc = 0.5 (u[i] + u[i - 1]), i periodic;   vc = 0.5 (v[j] + v[j - 1])
//     row -1: row H - 1 on a single domain (the model's pole-to-pole roll), a band's first north ghost row of v
//   words: u, v, theta, T, u u, v v, T T, uc vc, vc T, vc theta;  per row: p, p p
//
// Contraction is off for the whole file (the Makefile builds it with -ffp-contract=fast-honor-pragmas).
//
// The order of a row's sum is a function of W alone.  One 256-thread workgroup owns the row (j, k): lane t adds the
// terms i = t, t + 256, ... in that order onto 0.0; the 64 lanes of a wave combine by the xor butterfly 32, 16, .. 1
// (both partners add the same two numbers: every lane ends on the same bits); the four waves combine in wave order
// through LDS; one thread adds the row's sum into the accumulator word.  No atomics, no second launch, one writer per
// accumulator word per launch: the same state gives the same bits, whatever H, the band, the number of CUs or the
// number of levels a workgroup walks.
//
// The state's layout is [j][k][i]: a (j, k) row is one contiguous run and a wave requests 64 consecutive i.  A
// workgroup walks a segment of the levels of its row j: p of the row is read once, widened and parked in LDS (lane t
// reads back only what it wrote: no barrier), the Exner table sits in LDS too.  Per sample (3 L + 1) H W elements come
// from HBM at least; u[i - 1] comes from the lines u[i] brings, row j - 1 of v from whatever cache still holds what
// row j - 1's own workgroup requested -- not measured.
#pragma clang fp contract(off)
#include "pe25d_host.h"

#include "pe25d_climate.h"
#include "pe25d_phase_geometry.h"

namespace gcm {

// (kClThreads, kClBatch -- 256-column chunks requested together, then added in order: pe25d_phase_geometry.h)
constexpr int kClWaves = kClThreads / 64;
constexpr int kClRedDoubles = 2 * kClWaves * GCM_CLIM_WORDS3;   // two buffers of the waves' sums: one barrier per level

size_t climate_lds_bytes(int W) { return sizeof(double) * ((size_t)kExnerTabDoubles + kClRedDoubles + (size_t)W); }

// the workgroup's N sums, in thread n < N (word n): the butterfly, then the waves in order.  `red`: kClWaves * N
// doubles nobody else touches until the next barrier but one
template <int N>
__device__ __forceinline__ double cl_block_sum(double (&s)[N], double *red) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int n = 0; n < N; ++n) s[n] = s[n] + __shfl_xor(s[n], d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int n = 0; n < N; ++n) red[(threadIdx.x >> 6) * N + n] = s[n];
    }
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x < N) {
        r = red[threadIdx.x];
        for (int w = 1; w < kClWaves; ++w) r = r + red[w * N + threadIdx.x];
    }
    return r;
}

// grid (rows, level segments).  Every thread reaches every barrier: lanes beyond W add nothing
template <typename T>
__global__ __launch_bounds__(kClThreads) void pe_climate_kernel(ClimateArgs a) {
    extern __shared__ __align__(16) double cl_lds[];
    double *tab = cl_lds, *red = tab + kExnerTabDoubles, *prow = red + kClRedDoubles;
    for (int n = threadIdx.x; n < kExnerTabDoubles; n += kClThreads) tab[n] = a.exner_tab[n];
    __syncthreads();
    const int W = a.W, L = a.L, H = a.H;
    const int j = (int)blockIdx.x, seg = (int)blockIdx.y;
    const int t0 = (int)threadIdx.x;
    const int k0 = (int)((long)seg * L / a.nseg), k1 = (int)((long)(seg + 1) * L / a.nseg);
    const int jm = (a.wrap && j == 0) ? H - 1 : j - 1;
    const T *pj = (const T *)a.p + (long)j * W;
    double s2[GCM_CLIM_WORDS2] = {0.0, 0.0};
    for (int i = t0; i < W; i += kClThreads) {
        const double pc = (double)pj[i];
        prow[i] = pc;
        s2[0] = s2[0] + pc;
        s2[1] = s2[1] + pc * pc;
    }
    int flip = 0;
    if (seg == 0) {                                            // (wave-uniform: the row's p and p p, once)
        const double r = cl_block_sum<GCM_CLIM_WORDS2>(s2, red);
        if (t0 < GCM_CLIM_WORDS2) a.m2[(long)t0 * H + j] += r;
        flip = 1;
    }
    for (int k = k0; k < k1; ++k) {
        const T *ur = (const T *)a.u + ((long)j * L + k) * W;
        const T *vr = (const T *)a.v + ((long)j * L + k) * W;
        const T *vn = (const T *)a.v + ((long)jm * L + k) * W;
        const T *tr = (const T *)a.t + ((long)j * L + k) * W;
        const double sg = a.sig[k];
        double s[GCM_CLIM_WORDS3];
#pragma unroll
        for (int n = 0; n < GCM_CLIM_WORDS3; ++n) s[n] = 0.0;
        for (int ib = t0; ib < W; ib += kClBatch * kClThreads) {
            T xu[kClBatch], xw[kClBatch], xv[kClBatch], xn[kClBatch], xt[kClBatch];
#pragma unroll
            for (int b = 0; b < kClBatch; ++b) {
                const int i = ib + b * kClThreads;
                if (i >= W) break;
                xu[b] = ur[i];
                xw[b] = ur[i == 0 ? W - 1 : i - 1];
                xv[b] = vr[i];
                xn[b] = vn[i];
                xt[b] = tr[i];
            }
#pragma unroll
            for (int b = 0; b < kClBatch; ++b) {
                const int i = ib + b * kClThreads;
                if (i >= W) break;
                const double u = (double)xu[b], v = (double)xv[b], th = (double)xt[b];
                const double pl = sg * prow[i] + a.ptop;
                const double tt = th * exner(pl, tab);
                const double uc = 0.5 * (u + (double)xw[b]);
                const double vc = 0.5 * (v + (double)xn[b]);
                s[0] = s[0] + u;
                s[1] = s[1] + v;
                s[2] = s[2] + th;
                s[3] = s[3] + tt;
                s[4] = s[4] + u * u;
                s[5] = s[5] + v * v;
                s[6] = s[6] + tt * tt;
                s[7] = s[7] + uc * vc;
                s[8] = s[8] + vc * tt;
                s[9] = s[9] + vc * th;
            }
        }
        // (two buffers: the readers of this level's sums are past them before anyone writes this buffer again, which is
        // behind the next level's barrier)
        const double r = cl_block_sum<GCM_CLIM_WORDS3>(s, red + flip * (kClWaves * GCM_CLIM_WORDS3));
        flip ^= 1;
        if (t0 < GCM_CLIM_WORDS3) a.m3[((long)t0 * L + k) * H + j] += r;
    }
}

void launch_climate(ClimateArgs a, bool f32, int cus, hipStream_t s) {
    // the levels are split over the grid until some eight workgroups a CU are in flight; the sums do not depend on it
    a.nseg = phase_climate_nseg(a.H, a.L, cus);
    const dim3 grid((unsigned)a.H, (unsigned)a.nseg);
    const size_t lds = climate_lds_bytes(a.W);
    if (f32) hipLaunchKernelGGL(pe_climate_kernel<float>, grid, dim3(kClThreads), lds, s, a);
    else hipLaunchKernelGGL(pe_climate_kernel<double>, grid, dim3(kClThreads), lds, s, a);
}

// ---------------------------------------------------------------- the handle's side
// layout of PeClimate::buf (doubles): sig [L] | m3 [GCM_CLIM_WORDS3][L][H] | m2 [GCM_CLIM_WORDS2][H]
static size_t clim_m3(const Pe25d *m) { return (size_t)GCM_CLIM_WORDS3 * m->L * m->H; }
static size_t clim_m2(const Pe25d *m) { return (size_t)GCM_CLIM_WORDS2 * m->H; }

static int clim_hip(hipError_t e, const char *fn, std::string *err) {
    if (e == hipSuccess) return GCM_OK;
    *err = std::string("hip: ") + fn + ": " + hipGetErrorString(e);
    return GCM_ERR_HIP;
}
static int clim_registered(const Pe25d *m, const char *fn, std::string *err) {
    if (m->clim.every > 0) return GCM_OK;
    *err = std::string(fn) + ": no climatology registered (gcm_set_climate)";
    return GCM_ERR_STATE;
}

int pe25d_set_climate(Pe25d *m, int every, hipStream_t s, std::string *err) {
    PeClimate &z = m->clim;
    if (every < 0) { *err = "gcm_set_climate: every must be >= 0"; return GCM_ERR_ARG; }
    if (every == 0) {
        if (!z.buf) return GCM_OK;
        // (a sample may still be adding to the sums)
        if (int rc = clim_hip(hipStreamSynchronize(s), "gcm_set_climate", err)) return rc;
        m->allocs.erase(std::remove(m->allocs.begin(), m->allocs.end(), (void *)z.buf), m->allocs.end());
        (void)hipFree(z.buf);
        z = PeClimate{};
        return GCM_OK;
    }
    if (climate_lds_bytes(m->W) > 64 * 1024) {
        *err = "gcm_set_climate: a row of " + std::to_string(m->W) + " columns does not fit the sample's LDS";
        return GCM_ERR_UNSUPPORTED;
    }
    const size_t sums = clim_m3(m) + clim_m2(m);
    if (!z.buf) {
        std::vector<double> init((size_t)m->L + sums, 0.0);
        std::copy(m->sig_host.begin(), m->sig_host.end(), init.begin());
        if (!dev_upload<double>(m, &z.buf, init.data(), init.size())) { *err = "hip: gcm_set_climate allocation failed"; return GCM_ERR_HIP; }
    } else if (int rc = clim_hip(hipMemsetAsync(z.buf + m->L, 0, sizeof(double) * sums, s), "gcm_set_climate", err)) {
        return rc;
    }
    z.every = every;
    z.steps = 0;
    z.n = 0;
    return GCM_OK;
}

int pe25d_climate_every(const Pe25d *m) { return m->clim.every; }

bool pe25d_climate_due(Pe25d *m) {
    PeClimate &z = m->clim;
    if (z.every <= 0) return false;
    return ++z.steps % z.every == 0;
}

// The sample is a pure reader of the current state set on `s` and writes its own sums only: it leaves the column sums,
// the fork at the last K4 and the ghost-row bookkeeping as they are (unlike pe25d_hs_rows, which writes u and v).
// What must still hold is that whatever overwrites this state set later is ordered behind this launch.  The set is
// written again by the corrector's K4 two steps on, by the physics phases behind it, and -- a band -- by the unpack
// of the exchange that follows that K4 (its ghost rows, of which this launch reads v's row -1).  K4 of the rows the
// caller's stream keeps (all rows; a band: the interior rows) follows this launch in stream order on `s`.  A band's
// edge rows' K4 runs on the second stream, which every stage makes wait for its fork: the completion of the previous
// stage's K4 on `s` (ev_k4) or a record on `s` at the head of the stage (ev_fork) -- an event behind this launch on `s`
// in either case, from the very next stage on; the pack, the exchange and the unpack follow that K4 in stream order
// (or on streams that wait for the pack).  The third stream writes no state set.  The launches of the next stage that
// may run beside this one (chain B forked at ev_k4: K1, pit, column sums, anchors, the tracers) write intermediates
// and tracers only, none of which is read here.
int pe25d_climate_sample(Pe25d *m, hipStream_t s, std::string *err) {
    if (int rc = clim_registered(m, "gcm_climate_sample", err)) return rc;
    PeClimate &z = m->clim;
    const int set = m->cur_i;
    ClimateArgs a{};
    a.p = state_field(m, set, GCM_P); a.u = state_field(m, set, GCM_U);
    a.v = state_field(m, set, GCM_V); a.t = state_field(m, set, GCM_T);
    a.sig = z.buf; a.exner_tab = m->exner_tab;
    a.m3 = z.buf + m->L; a.m2 = a.m3 + clim_m3(m);
    a.ptop = m->cfg.ptop;
    a.W = m->W; a.H = m->H; a.L = m->L; a.wrap = m->wrap ? 1 : 0;
    launch_climate(a, m->f32, m->cus, s);
    if (int rc = clim_hip(hipGetLastError(), "gcm_climate_sample", err)) return rc;
    ++z.n;
    return GCM_OK;
}

int pe25d_climate_reset(Pe25d *m, hipStream_t s, std::string *err) {
    if (int rc = clim_registered(m, "gcm_climate_reset", err)) return rc;
    PeClimate &z = m->clim;
    if (int rc = clim_hip(hipMemsetAsync(z.buf + m->L, 0, sizeof(double) * (clim_m3(m) + clim_m2(m)), s), "gcm_climate_reset", err)) return rc;
    z.n = 0;
    return GCM_OK;
}

int pe25d_get_climate(Pe25d *m, double *m3, double *m2, int64_t *nsamples, hipStream_t s, std::string *err) {
    if (int rc = clim_registered(m, "gcm_get_climate", err)) return rc;
    const PeClimate &z = m->clim;
    hipError_t e = hipSuccess;
    if (m3) e = hipMemcpyAsync(m3, z.buf + m->L, sizeof(double) * clim_m3(m), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && m2) e = hipMemcpyAsync(m2, z.buf + m->L + clim_m3(m), sizeof(double) * clim_m2(m), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (int rc = clim_hip(e, "gcm_get_climate", err)) return rc;
    if (nsamples) *nsamples = z.n;
    return GCM_OK;
}

int pe25d_put_climate(Pe25d *m, const double *m3, const double *m2, int64_t nsamples, hipStream_t s, std::string *err) {
    if (int rc = clim_registered(m, "gcm_put_climate", err)) return rc;
    if (!m3 || !m2 || nsamples < 0) { *err = "gcm_put_climate: m3 and m2 are required, nsamples must be >= 0"; return GCM_ERR_ARG; }
    PeClimate &z = m->clim;
    hipError_t e = hipMemcpyAsync(z.buf + m->L, m3, sizeof(double) * clim_m3(m), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(z.buf + m->L + clim_m3(m), m2, sizeof(double) * clim_m2(m), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);          // (the caller's arrays are free again when the call returns)
    if (int rc = clim_hip(e, "gcm_put_climate", err)) return rc;
    z.n = nsamples;
    return GCM_OK;
}

}  // namespace gcm

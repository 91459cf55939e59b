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
// layout of the sampler's buf (doubles): sig [L] | m3 [GCM_CLIM_WORDS3][L][H] | m2 [GCM_CLIM_WORDS2][H].  every, due, reset,
// get, put and free are the samplers' shared routines (pe25d_sampler_*, pe25d_state.hip)

// A second registration zeroes the sums in place: the buffer's size is the handle's own
int pe25d_set_climate(Pe25d *m, int every, hipStream_t s, std::string *err) {
    PeSampler &z = m->clim;
    if (every < 0) { *err = "gcm_set_climate: every must be >= 0"; return GCM_ERR_ARG; }
    if (every == 0) {
        if (!z.buf) return GCM_OK;
        // (a sample may still be adding to the sums)
        if (int rc = hip_rc(hipStreamSynchronize(s), "gcm_set_climate", err)) return rc;
        pe25d_sampler_free(m, kSampleClimate);
        return GCM_OK;
    }
    if (climate_lds_bytes(m->W) > 64 * 1024) {
        *err = "gcm_set_climate: a row of " + std::to_string(m->W) + " columns does not fit the sample's LDS";
        return GCM_ERR_UNSUPPORTED;
    }
    const size_t m3 = (size_t)GCM_CLIM_WORDS3 * m->L * m->H, m2 = (size_t)GCM_CLIM_WORDS2 * m->H;
    if (!z.buf) {
        std::vector<double> init((size_t)m->L + m3 + m2, 0.0);
        std::copy(m->sig_host.begin(), m->sig_host.end(), init.begin());
        if (!dev_upload<double>(m, &z.buf, init.data(), init.size())) { *err = "hip: gcm_set_climate allocation failed"; return GCM_ERR_HIP; }
    } else if (int rc = hip_rc(hipMemsetAsync(z.buf + m->L, 0, sizeof(double) * (m3 + m2), s), "gcm_set_climate", err)) {
        return rc;
    }
    z.head = (size_t)m->L;
    z.words[0] = m3;
    z.words[1] = m2;
    z.every = every;
    z.steps = 0;
    z.n = 0;
    return GCM_OK;
}

// The launch reads p, u, v and theta of the current state set, and on a band v's first north ghost row; how it is
// ordered against the stages that follow: pe25d_kernels.h, at the samplers' declarations
int pe25d_climate_sample(Pe25d *m, hipStream_t s, std::string *err) {
    if (int rc = pe25d_sampler_registered(m, kSampleClimate, "gcm_climate_sample", err)) return rc;
    PeSampler &z = m->clim;
    const int set = m->cur_i;
    ClimateArgs a{};
    a.p = state_field(m, set, GCM_P); a.u = state_field(m, set, GCM_U);
    a.v = state_field(m, set, GCM_V); a.t = state_field(m, set, GCM_T);
    a.sig = z.buf; a.exner_tab = m->exner_tab;
    a.m3 = z.buf + z.head; a.m2 = a.m3 + z.words[0];
    a.ptop = m->cfg.ptop;
    a.W = m->W; a.H = m->H; a.L = m->L; a.wrap = m->wrap ? 1 : 0;
    launch_climate(a, m->f32, m->cus, s);
    if (int rc = hip_rc(hipGetLastError(), "gcm_climate_sample", err)) return rc;
    ++z.n;
    return GCM_OK;
}

}  // namespace gcm

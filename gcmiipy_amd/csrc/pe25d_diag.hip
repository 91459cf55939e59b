// GCM_PE25D diagnostics and taps: calc_energy + STATS (gcm_stats), the polar filter of a field (gcm_polar_filter), the
// stage's intermediates (gcm_get_intermediate), and the small queries gcm_diag.hip and the tools take: the filter plan,
// the total variation's shapes, a field's address, the timing events.  Nothing here belongs to a stage; the handle:
// pe25d_host.h.
#include "pe25d_host.h"

namespace gcm {

using PeArgs = PeArgsT<double>;   // the diagnostics and the column physics below are fp64 only

// ---------------------------------------------------------------- calc_energy + STATS (no_limits_2_5d.py:35-60,85-91)
// thread per (j,i) column; out[kStatsWords*block + {0,1,2}] = partial sums of ke, ate, geo,
// {3,4,5,6} = max u, min u, max v, min v of the block's columns (fmax / fmin: a NaN drops out), {7} = cells where u or
// v is NaN, {8,9} = cells where u is, where v is: the host makes a field's extrema NaN from the field's own count
constexpr int kStatsWords = 10;
__global__ __launch_bounds__(256) void pe_energy_kernel(PeArgs a, const double *area, int area_by_i,
                                                        double *out) {
    __shared__ double tab[kExnerTabDoubles];
    __shared__ double red[kStatsWords][4];
    tab[threadIdx.x] = a.exner_tab[threadIdx.x];
    __syncthreads();
    const Idx ix{a.W, a.H, a.L, a.wrap};
    const int W = a.W, L = a.L;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int j = blockIdx.y;
    double ke = 0.0, ate = 0.0, geo = 0.0;
    double umax = -INFINITY, umin = INFINITY, vmax = -INFINITY, vmin = INFINITY, nn = 0.0, nu = 0.0, nv = 0.0;
    if (i < W) {
        const int iw = i == 0 ? W - 1 : i - 1;
        const double pc = a.p[ix.r2(j) + i];
        const double ar = area[area_by_i ? i : 0];   // geom.area (H,) broadcasts along the LAST axis (:49)
        const long c3 = ix.r3(j), n3 = ix.r3(j - 1);
        double depth = 0.0;
        for (int k = 0; k < L; ++k) {
            const long o = c3 + (long)k * W;
            const double u_c = a.u[o + i], v_c = a.v[o + i];
            umax = fmax(umax, u_c); umin = fmin(umin, u_c);
            vmax = fmax(vmax, v_c); vmin = fmin(vmin, v_c);
            if (u_c != u_c || v_c != v_c) nn += 1.0;
            if (u_c != u_c) nu += 1.0;
            if (v_c != v_c) nv += 1.0;
            const double uc = (u_c + a.u[o + iw]) * 0.5;                          // imh(u)
            const double vc = (v_c + a.v[n3 + (long)k * W + i]) * 0.5;            // jmh(v)
            const double mag = sqrt(uc * uc + vc * vc);
            const double tp = pc * a.sig[k] + a.ptop;
            const double tt = a.t[o + i] * exner(tp, tab);
            const double rho = tp / (kRd * tt);
            const double gd = (pc * a.dsig[k]) / (rho * kG);
            const double airmass = rho * gd * ar;
            depth += gd;                                                          // cumsum over k
            geo += depth * airmass * kG;
            ke += mag * mag * .5 * airmass;
            ate += tt * kCp * airmass;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        ke += __shfl_down(ke, o);
        ate += __shfl_down(ate, o);
        geo += __shfl_down(geo, o);
        umax = fmax(umax, __shfl_down(umax, o)); umin = fmin(umin, __shfl_down(umin, o));
        vmax = fmax(vmax, __shfl_down(vmax, o)); vmin = fmin(vmin, __shfl_down(vmin, o));
        nn += __shfl_down(nn, o);
        nu += __shfl_down(nu, o);
        nv += __shfl_down(nv, o);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][w] = ke; red[1][w] = ate; red[2][w] = geo;
        red[3][w] = umax; red[4][w] = umin; red[5][w] = vmax; red[6][w] = vmin; red[7][w] = nn;
        red[8][w] = nu; red[9][w] = nv;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double *o = out + kStatsWords * ((long)blockIdx.y * gridDim.x + blockIdx.x);
        for (int q = 0; q < 3; ++q) o[q] = red[q][0] + red[q][1] + red[q][2] + red[q][3];
        o[3] = fmax(fmax(red[3][0], red[3][1]), fmax(red[3][2], red[3][3]));
        o[4] = fmin(fmin(red[4][0], red[4][1]), fmin(red[4][2], red[4][3]));
        o[5] = fmax(fmax(red[5][0], red[5][1]), fmax(red[5][2], red[5][3]));
        o[6] = fmin(fmin(red[6][0], red[6][1]), fmin(red[6][2], red[6][3]));
        for (int q = 7; q < kStatsWords; ++q) o[q] = red[q][0] + red[q][1] + red[q][2] + red[q][3];
    }
}

// low_pass.arakawa_1977 on a field of the handle's grid, nlev <= L levels, host [nlev][H][W] in and
// out: the spu filter kernel with iph(sp) = 1 (su * 1 is exact).  spu, pgfu and pit serve as scratch
// -- every stage rewrites them before it reads them.
template <typename T>
__global__ void pe_fill_kernel(T *dst, long n, T x) {
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) dst[e] = x;
}
template <typename T>
static int filter_field_t(Pe25d *m, int nlev, const double *in, double *out, hipStream_t s, std::string *err) {
    PeBufs<T> &B = bufs<T>(m);
    const int W = m->W, H = m->H;
    m->last_stage_set = -1;                      // spu, pgfu and pit are scratch here: the parity tap has nothing to return
    m->k4_fork_valid = false;
    hipError_t e = field_to_device(m, B.pgfu, in, nlev, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pe_fill_kernel<T>, dim3(256), dim3(256), 0, s, B.pit, (long)H * W, T(1.0));
        PeArgsT<T> a = make_args<T>(m, m->cur_i, m->cur_i, 0.0);
        a.L = nlev;
        a.sp = B.pit;
        a.su = B.pgfu;
        a.spu = B.spu;
        a.filter = 1;
        a.j0 = 0;
        a.j1 = H;
        const int fft_threads = m->cplan.ok ? m->cplan.threads : kFftThreads;
        hipLaunchKernelGGL(spu_filter_kernel_for<T>(m->cplan), dim3(H, (nlev + 1) / 2), dim3(fft_threads),
                           filter_lds_bytes<T>(m), s, a);
        e = field_to_host(m, out, B.spu, nlev, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) {
        *err = std::string("pe25d polar filter: ") + hipGetErrorString(e);
        return GCM_ERR_HIP;
    }
    return GCM_OK;
}

// ---------------------------------------------------------------- parity tap: the stage's intermediates
// phi on every level in the host layout [k][j][i], float64: the stored anchors on the even levels, the odd
// levels stepped up from them with phi_up -- the expression K3 and K4 evaluate
template <typename T>
__global__ __launch_bounds__(256) void pe_phi_full_kernel(PeArgsT<T> a, double *out) {
    __shared__ double tab[kExnerTabDoubles];
    for (int n = threadIdx.x; n < kExnerTabDoubles; n += 256) tab[n] = a.exner_tab[n];
    __syncthreads();
    const int W = a.W, H = a.H, L = a.L;
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= W) return;
    const long c3 = (long)j * L * W + i;
    const T spc = a.sp[(long)j * W + i];
    T phi_lo = T(0.0), t_lo = T(0.0), ex_lo = T(0.0);
    for (int k = 0; k < L; ++k) {
        const T t = a.st[c3 + (long)k * W];
        const T ex = exner(spc * a.sig[k] + a.ptop, tab);
        const T phi = (k & 1) ? phi_up(phi_lo, t_lo, t, ex_lo, ex) : a.phi[c3 + (long)k * W];
        out[((long)k * H + j) * W + i] = (double)phi;
        phi_lo = phi; t_lo = t; ex_lo = ex;
    }
}

template <typename T>
static int intermediate_t(Pe25d *m, int kind, double *out, hipStream_t s, std::string *err) {
    PeBufs<T> &B = bufs<T>(m);
    const int W = m->W, H = m->H, L = m->L;
    const T *src = nullptr;
    int lev = L;
    switch (kind) {
        case GCM_INT_SPU: src = B.spu; break;
        case GCM_INT_PGFU: src = B.pgfu; break;
        case GCM_INT_PIT: src = B.pit; lev = 1; break;
        case GCM_INT_PN: src = B.pn; lev = 1; break;
        case GCM_INT_PHI: break;
        default: *err = "gcm_get_intermediate: unknown kind"; return GCM_ERR_ARG;
    }
    if (kind == GCM_INT_PHI) {
        PeArgsT<T> a = make_args<T>(m, m->last_stage_set, m->last_stage_set, 0.0);
        hipLaunchKernelGGL(pe_phi_full_kernel<T>, dim3((W + 255) / 256, H), dim3(256), 0, s, a, m->stage3);
    }
    // (the other kinds are fields of the device layout: the transpose and the copy of pe25d_state.hip)
    hipError_t e = kind == GCM_INT_PHI ? hipMemcpyAsync(out, m->stage3, sizeof(double) * (size_t)lev * H * W, hipMemcpyDeviceToHost, s)
                                       : field_to_host(m, out, src, lev, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) {
        *err = std::string("gcm_get_intermediate: ") + hipGetErrorString(e);
        return GCM_ERR_HIP;
    }
    return GCM_OK;
}

int pe25d_intermediate(Pe25d *m, int kind, double *out, hipStream_t s, std::string *err) {
    if (!m->wrap) { *err = "gcm_get_intermediate: single band only"; return GCM_ERR_UNSUPPORTED; }
    if (m->last_stage_set < 0) { *err = "gcm_get_intermediate: no half step taken yet"; return GCM_ERR_STATE; }
    if (m->aux) (void)hipStreamSynchronize(m->aux);
    return m->f32 ? intermediate_t<float>(m, kind, out, s, err) : intermediate_t<double>(m, kind, out, s, err);
}

int pe25d_filter_field(Pe25d *m, int nlev, const double *in, double *out, hipStream_t s, std::string *err) {
    if (nlev < 1 || nlev > m->L) {
        *err = "polar filter: 1 <= levels <= the handle's layers";
        return GCM_ERR_ARG;
    }
    if (!m->cfg.filter && m->W > 1) {
        *err = "polar filter: the handle was created with filter = 0";
        return GCM_ERR_UNSUPPORTED;
    }
    if (m->W == 1) {                                    // low_pass.py:58-59: identity
        if (out != in) memcpy(out, in, sizeof(double) * (size_t)nlev * m->H);
        return GCM_OK;
    }
    return m->f32 ? filter_field_t<float>(m, nlev, in, out, s, err) : filter_field_t<double>(m, nlev, in, out, s, err);
}

// calc_energy + STATS in one launch and one synchronisation of `s`: out9 = u_max, u_min, v_max,
// v_min, ke, ate, geo, total, the number of cells where u or v is NaN.  The area table and the partials live in the
// handle.  The call does not join the second stream, and need not: only single domains get here, whose state sets are
// written by K4 (update_whole) and by the phases behind the dynamics (pe_phase_rows), all of them on the caller's stream
// `s`; a single domain's second stream carries K1 + pit (spu, pit, p_n: scratch this kernel does not read) and the
// tracer launches (the tracers' own fields), see half_t and stage_tracers in pe25d_kernels.hip.  The kernel below follows
// every writer of p, u, v and theta in stream order.
int pe25d_stats(Pe25d *m, const double *area_host, int area_len, double out[9], hipStream_t s, std::string *err) {
    if (m->f32) { *err = "gcm_energy / gcm_stats: fp64 handles only"; return GCM_ERR_UNSUPPORTED; }
    if (!m->wrap) { *err = "gcm_energy / gcm_stats: single band only"; return GCM_ERR_UNSUPPORTED; }
    if (!(area_len == 1 || area_len == m->W)) {
        *err = "gcm_energy: geom.area (H,) must broadcast against the last axis W (no_limits_2_5d.py:49): "
               "needs H == W or H == 1";
        return GCM_ERR_ARG;
    }
    const int gx = (m->W + 255) / 256, nb = gx * m->H;
    if (!m->stats_dev) {
        if (!dev_upload<double>(m, &m->stats_dev, nullptr, (size_t)kStatsWords * nb + m->W)) {
            *err = "hip: gcm_stats allocation failed";
            return GCM_ERR_HIP;
        }
        m->stats_host.resize((size_t)kStatsWords * nb);
    }
    double *d_area = m->stats_dev + (size_t)kStatsWords * nb;
    if (m->area_host.size() != (size_t)area_len || memcmp(m->area_host.data(), area_host, sizeof(double) * area_len)) {
        m->area_host.assign(area_host, area_host + area_len);
        if (hipMemcpyAsync(d_area, m->area_host.data(), sizeof(double) * area_len, hipMemcpyHostToDevice, s) != hipSuccess) {
            *err = "hip: gcm_stats area upload failed";
            return GCM_ERR_HIP;
        }
    }
    PeArgs a = make_args<double>(m, m->cur_i, m->cur_i, 0.0);
    hipLaunchKernelGGL(pe_energy_kernel, dim3(gx, m->H), dim3(256), 0, s, a, d_area, area_len > 1 ? 1 : 0, m->stats_dev);
    double *part = m->stats_host.data();
    if (hipMemcpyAsync(part, m->stats_dev, sizeof(double) * kStatsWords * nb, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        *err = "hip: gcm_stats kernel failed";
        return GCM_ERR_HIP;
    }
    double ke = 0, ate = 0, geo = 0, nn = 0, nu = 0, nv = 0, umax = -INFINITY, umin = INFINITY, vmax = -INFINITY, vmin = INFINITY;
    for (int b = 0; b < nb; ++b) {
        const double *o = part + (size_t)kStatsWords * b;
        ke += o[0]; ate += o[1]; geo += o[2]; nn += o[7]; nu += o[8]; nv += o[9];
        umax = std::fmax(umax, o[3]); umin = std::fmin(umin, o[4]);
        vmax = std::fmax(vmax, o[5]); vmin = std::fmin(vmin, o[6]);
    }
    // np.max / np.min propagate NaN, each of its own field (no_limits_2_5d.py:85-88): a NaN in v leaves u_max finite
    out[0] = nu > 0 ? NAN : umax; out[1] = nu > 0 ? NAN : umin; out[2] = nv > 0 ? NAN : vmax; out[3] = nv > 0 ? NAN : vmin;
    out[4] = ke; out[5] = ate; out[6] = geo; out[7] = ke + ate + geo; out[8] = nn;
    return GCM_OK;
}

// field geometry for get_total_variation (axis 0 of the reference layout): 2-D p differences rows,
// the 3-D fields difference levels inside a row slab
int pe25d_filter_plan(int n, unsigned *out, int cap) {
    if (!out || n < 2 || cap < 3 + 4 * kMaxSuper) return GCM_ERR_ARG;
    SuperPlan P;
    make_super_plan(n, &P);
    out[0] = (unsigned)P.ok;
    out[1] = (unsigned)P.npass;
    out[2] = (unsigned)P.threads;
    for (int p = 0; p < kMaxSuper; ++p) {
        out[3 + 4 * p] = (unsigned)P.r1[p];
        out[4 + 4 * p] = (unsigned)P.r2[p];
        out[5 + 4 * p] = P.magic[p];
        out[6 + 4 * p] = P.imagic[p];
    }
    return GCM_OK;
}

void pe25d_tv_shape(const Pe25d *m, int field, long *n_outer, long *n_axis, long *n_inner, int *wrap) {
    if (field == GCM_P) { *n_outer = 1; *n_axis = m->H; *n_inner = m->W; *wrap = m->wrap ? 1 : 0; }
    else { *n_outer = m->H; *n_axis = m->L; *n_inner = m->W; *wrap = 1; }
}

// current-state field for the diagnostics reductions; *f32 tells the element type
const void *pe25d_field(Pe25d *m, int field, long *n, int *f32) {
    *n = (long)m->H * m->W * (field == GCM_P ? 1 : m->L);
    *f32 = m->f32 ? 1 : 0;
    return state_field(m, m->cur_i, field);
}

void pe25d_timing(Pe25d *m, std::vector<hipEvent_t> *ev, size_t *used) {
    m->ev = ev;
    m->ev_used = used;
}

}  // namespace gcm

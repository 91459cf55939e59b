// Passive tracers of GCM_PE25D under a transport scheme (gcm_set_tracer_scheme): the donor-cell and the van Leer
// limited forms of the tracer march of pe25d_tracer.h, and their picker.  Included by pe25d_tracer_lim_f64.hip /
// pe25d_tracer_lim_f32.hip only.
//
// The update keeps the flux form, the mass fluxes and the divisor of the centred kernel,
//   c_n = (c p - (adq + dqs) dt) / p_n,
// and changes only the value of the stage tracer sc that each mass flux carries through its face.  For a face with
// mass flux F between cells A and B (F > 0 carries mass from A to B):
//   U = A if F > 0 (strict, as donor_cell_flux, flux_limiter.py:24) else B, D = the other, UU = the cell next to U
//   on the side away from the face;
//   GCM_TRACER_UPWIND:   face value = sc[U]
//   GCM_TRACER_VANLEER:  face value = sc[U] + 1/2 phi(r) (sc[D] - sc[U]),  phi(r) = (r + |r|) / (1 + |r|),
//                        r = (sc[U] - sc[UU]) / (sc[D] - sc[U]), 0 where the denominator is 0 (calc_r)
// i.e. F_low + phi (F_high - F_low) with F_high the centred flux, as the 2-D kernels compose it (gcm_math.h,
// face_flux).  Plain differences of neighbouring cells (no dx or dsigma weights); all three directions from the one
// stage field (the Matsuno stages are not split).  i is periodic, j goes through Idx as in the centred kernel, the
// column does not wrap: a level face whose UU lies outside 0 .. L-1 is donor-cell.  sigma-dot at face k (between
// levels k - 1 and k) carries mass from level k - 1 into level k when positive: the update adds
// (flux[k] - flux[k + 1]) dt / dsig[k].  The level flux stays a rounded product carried from the level above.
#pragma once
#include "../../include/gcmcore.h"
#include "pe25d_dev.h"

namespace gcm {

// the value of sc a face carries: cells aa | a || b | bb along the axis, F > 0 from a to b.  ok_aa / ok_bb: the far
// cell on that side exists (level faces).  1/2 phi(r) = |num| / (|d| + |num|) where num d > 0, else 0: one
// reciprocal, no division by d (gcm_math.h, face_flux); it never exceeds 1, the clamp only keeps a sum of
// denormals from reaching the result as an infinity
template <int SCHEME, typename T>
__device__ __forceinline__ T tracer_face(T F, T q_aa, T q_a, T q_b, T q_bb, bool ok_aa = true, bool ok_bb = true) {
    const bool pos = F > T(0.0);
    const T q_u = pos ? q_a : q_b;
    if (SCHEME != GCM_TRACER_VANLEER) return q_u;
    const T q_d = pos ? q_b : q_a, q_uu = pos ? q_aa : q_bb;
    const bool ok = pos ? ok_aa : ok_bb;
    const T d = q_d - q_u, num = q_u - q_uu;
    const T an = fabs(num), ad = fabs(d);
    const bool rpos = ok && ((sign_word(num) ^ sign_word(d)) >= 0) && an > T(0.0) && ad > T(0.0);
    const T hphi = rpos ? fmin(an * rcp(ad + an), T(1.0)) : T(0.0);
    return fma(hphi, d, q_u);
}
// face value x sigma-dot: a rounded product, as face_flux_v
template <typename T>
__device__ __forceinline__ T mul_rn(T a, T b) {
#pragma clang fp contract(off)
    return a * b;
}

// One thread per (j, i) column marching down the levels, NC tracers per launch chunk sharing spu, sv, pit and the
// rebuilt sigma-dot: the launch geometry, the tile order and the request form (scalar base + one 32-bit lane offset)
// are those of pe_tracer_kernel.  VANLEER adds the requests i -+ 2 and j -+ 2 per level and keeps a window of four
// levels of the own column (k + 1, k, k - 1, k - 2) in registers: one new request per level (k - 2).
template <typename T, int SCHEME, int NC, bool SAME>
__global__ __launch_bounds__(kTrCols * kTrRows) void pe_tracer_lim_kernel(TracerArgsT<T> a) {
    constexpr bool VL = SCHEME == GCM_TRACER_VANLEER;
    const Idx ix{a.W, a.H, a.L, a.wrap};
    const int W = a.W, L = a.L;
    const int ncol = (W + kTrCols - 1) / kTrCols;
    const int n0 = a.j1 - a.j0, nrows = n0 + (a.jb1 - a.jb0);
    const int ntiles = ncol * ((nrows + kTrRows - 1) / kTrRows);
    const int per_xcd = (int)(gridDim.x / 8);
    const int tile = (int)(blockIdx.x % 8) * per_xcd + (int)(blockIdx.x / 8);
    if (tile >= ntiles) return;
    const int rg = tile / ncol, ct = tile - rg * ncol;
    const int i = ct * kTrCols + (int)(threadIdx.x % kTrCols);
    const int r = rg * kTrRows + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kTrCols));
    if (i >= W || r >= nrows) return;
    const int j = r < n0 ? a.j0 + r : a.jb0 + (r - n0);
    const int iw = i == 0 ? W - 1 : i - 1, ie = i + 1 == W ? 0 : i + 1;
    const int iww = iw == 0 ? W - 1 : iw - 1, iee = ie + 1 == W ? 0 : ie + 1;
    const long toff = (long)blockIdx.y * NC * a.tstride;
    const T *c = a.c + toff, *sc = a.sc + toff;
    T *oc = a.oc + toff;
    const auto sbase = [](const T *p) {
        unsigned long long v = (unsigned long long)p;
        unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
        asm volatile("" : "+s"(lo), "+s"(hi));
        return (__attribute__((address_space(1))) char *)(((unsigned long long)hi << 32) | lo);
    };
    const unsigned ob_c = (unsigned)i * (unsigned)sizeof(T), ob_w = (unsigned)iw * (unsigned)sizeof(T),
                   ob_e = (unsigned)ie * (unsigned)sizeof(T), ob_ww = (unsigned)iww * (unsigned)sizeof(T),
                   ob_ee = (unsigned)iee * (unsigned)sizeof(T);
    const auto at = [sbase](const T *base, unsigned ol) { return *(const __attribute__((address_space(1))) T *)(sbase(base) + ol); };

    const int jg_row = wrapi(a.row0 + j, a.Hg);
    const T inv_dxj = a.inv_dxj[jg_row], inv_dy = a.inv_dy, dt = a.dt;
    const long p_n = ix.r2(j - 1), p_c = ix.r2(j), p_s = ix.r2(j + 1);
    const T sp_c = a.sp[p_c + i], sp_s = a.sp[p_s + i], sp_n = a.sp[p_n + i];
    const T jph_c = (sp_c + sp_s) * T(0.5), jph_n = (sp_n + sp_c) * T(0.5);
    const T pb_c = a.p[p_c + i];
    const T inv_pn = rcp(a.pn[p_c + i]);
    const T pit_c = a.pit[p_c + i];
    const long rn = ix.r3(j - 1), rc = ix.r3(j), rs = ix.r3(j + 1);
    // (VANLEER: rows j -+ 2 wrap through Idx on a single domain; on a band they are plain row arithmetic into the two
    // ghost rows a side that gcm_set_band_tracer_rows declared -- gcm_set_tracer_scheme refuses the scheme without them)
    const long rnn = VL ? ix.r3(j - 2) : rn, rss = VL ? ix.r3(j + 2) : rs;

    // running sum of conv from the top, per tracer the flux through the upper face of the level, and the own
    // column's window: sq_c = level k, sq_m = level k - 1 (VANLEER: carried), sq_p = level k + 1 (VANLEER)
    T rc_c = T(0.0);
    T fq_up[NC], sq_c[NC], sq_m[NC], sq_p[NC];
#pragma unroll
    for (int n = 0; n < NC; ++n) {
        fq_up[n] = T(0.0);
        sq_c[n] = at(sc + n * a.tstride + rc + (long)(L - 1) * W, ob_c);
        sq_p[n] = sq_c[n];                                       // (no level L: ok_bb is false there)
        if (VL) sq_m[n] = at(sc + n * a.tstride + rc + (long)(L > 1 ? L - 2 : 0) * W, ob_c);
    }
#pragma unroll 1
    for (int k = L - 1; k >= 0; --k) {
        // the level this march requests of the own column: k - 1 (UPWIND, as the centred kernel), k - 2 (VANLEER);
        // below level 0 any finite value (sd[0] = 0; a missing far cell is switched off by ok_aa)
        const long kc = (long)k * W, kq = VL ? (k > 1 ? kc - 2 * W : 0) : (k > 0 ? kc - W : kc);
        unsigned oc_, ow_, oe_, oww_, oee_;
        oc_ = ob_c; ow_ = ob_w; oe_ = ob_e; oww_ = ob_ww; oee_ = ob_ee;
        asm volatile("" : "+v"(oc_), "+v"(ow_), "+v"(oe_), "+v"(oww_), "+v"(oee_));
        const T spu_c = at(a.spu + rc + kc, oc_), spu_w = at(a.spu + rc + kc, ow_);
        const T sv_c = at(a.sv + rc + kc, oc_), sv_n = at(a.sv + rn + kc, oc_);
        const T spv_c = sv_c * jph_c, spv_n = sv_n * jph_n;
        // ---- aflux, dynamics.py:35-46: sigma-dot at (j, i), as K4 forms it
        const T dsg = a.dsig[k], sgb = a.sigb[k];
        T sd_c = T(0.0);                                         // sd[0] = 0, dynamics.py:44
        if (k > 0) {
            rc_c = conv_acc(rc_c, spu_c, spu_w, inv_dxj, sv_c, jph_c, sv_n, jph_n, inv_dy, dsg);
            sd_c = sd_of(rc_c, pit_c, sgb);
        }
        const T inv_ds = a.inv_dsig[k];
        // all requests of the level first (the stores below may alias the base tracer, see pe_tracer_kernel)
        T sq_e[NC], sq_w[NC], sq_n[NC], sq_s[NC], sq_ee[NC], sq_ww[NC], sq_nn[NC], sq_ss[NC], sq_q[NC], bq_c[NC];
#pragma unroll
        for (int n = 0; n < NC; ++n) {
            const T *s = sc + n * a.tstride;
            sq_e[n] = at(s + rc + kc, oe_); sq_w[n] = at(s + rc + kc, ow_);
            sq_n[n] = at(s + rn + kc, oc_); sq_s[n] = at(s + rs + kc, oc_);
            if (VL) {
                sq_ee[n] = at(s + rc + kc, oee_); sq_ww[n] = at(s + rc + kc, oww_);
                sq_nn[n] = at(s + rnn + kc, oc_); sq_ss[n] = at(s + rss + kc, oc_);
            } else {
                sq_ee[n] = sq_e[n]; sq_ww[n] = sq_w[n]; sq_nn[n] = sq_n[n]; sq_ss[n] = sq_s[n];   // (not read)
            }
            sq_q[n] = at(s + rc + kq, oc_);
            bq_c[n] = SAME ? sq_c[n] : at(c + n * a.tstride + rc + kc, oc_);
        }
#pragma unroll
        for (int n = 0; n < NC; ++n) {
            const T sq_mm = sq_q[n];                             // level k - 2 (VANLEER only)
            if (!VL) sq_m[n] = sq_q[n];
            // ---- advec_t, dynamics.py:174-181, on the scheme's face values: east (i | i + 1) and west, south
            // (j | j + 1) and north
            const T f_e = tracer_face<SCHEME>(spu_c, sq_w[n], sq_c[n], sq_e[n], sq_ee[n]);
            const T f_w = tracer_face<SCHEME>(spu_w, sq_ww[n], sq_w[n], sq_c[n], sq_e[n]);
            const T f_s = tracer_face<SCHEME>(spv_c, sq_n[n], sq_c[n], sq_s[n], sq_ss[n]);
            const T f_n = tracer_face<SCHEME>(spv_n, sq_nn[n], sq_n[n], sq_c[n], sq_s[n]);
            const T adq = (spu_c * f_e - spu_w * f_w) * inv_dxj + (spv_c * f_s - spv_n * f_n) * inv_dy;
            // ---- advec_sig, dynamics.py:49-52: face k between levels k - 1 (A) and k (B)
            const T f_k = tracer_face<SCHEME>(sd_c, sq_mm, sq_m[n], sq_c[n], sq_p[n], k > 1, k + 1 < L);
            const T fq = mul_rn(f_k, sd_c);
            const T dqs = -((fq - fq_up[n]) * inv_ds);
            fq_up[n] = fq;
            const T q_n = (bq_c[n] * pb_c - (adq + dqs) * dt) * inv_pn;
            *(__attribute__((address_space(1))) T *)(sbase(oc + n * a.tstride + rc + kc) + oc_) = q_n;
            sq_p[n] = sq_c[n];
            sq_c[n] = sq_m[n];
            if (VL) sq_m[n] = sq_mm;
        }
    }
}

template <typename T, int SCHEME>
static TracerKernel<T> tracer_lim_kernel_of(int nc, bool same) {
    if (nc == 4) return same ? pe_tracer_lim_kernel<T, SCHEME, 4, true> : pe_tracer_lim_kernel<T, SCHEME, 4, false>;
    if (nc == 2) return same ? pe_tracer_lim_kernel<T, SCHEME, 2, true> : pe_tracer_lim_kernel<T, SCHEME, 2, false>;
    return same ? pe_tracer_lim_kernel<T, SCHEME, 1, true> : pe_tracer_lim_kernel<T, SCHEME, 1, false>;
}

// scheme = GCM_TRACER_UPWIND or GCM_TRACER_VANLEER, chunks of nc = 4, 2 or 1 tracers (pe25d_tracers.hip,
// launch_tracers); instantiated in pe25d_tracer_lim_f{64,32}.hip
template <typename T>
TracerKernel<T> tracer_lim_kernel_for(int scheme, int nc, bool same) {
    return scheme == GCM_TRACER_VANLEER ? tracer_lim_kernel_of<T, GCM_TRACER_VANLEER>(nc, same)
                                        : tracer_lim_kernel_of<T, GCM_TRACER_UPWIND>(nc, same);
}

}  // namespace gcm

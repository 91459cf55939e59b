// Passive tracers of GCM_PE25D (see pe25d_kernels.hip, half_t): the tracer kernel and its picker.  Included by
// pe25d_tracer_f64.hip / pe25d_tracer_f32.hip only.
//
// A tracer c advances in each Matsuno stage with exactly the update the reference applies to q
// (dynamics.py:219 with advec_t :174-181 and advec_sig :49-52):
//   c_n = (c p - (advec_t(spu, spv, sc) + advec_sig(sd, sc)) dt) / p_n
// sc = the stage value of the tracer.  The kernel is its own launch beside K4, on chain B right behind K1 + pit,
// and reads only what the stage has produced already: spu (filtered, K1), sv and sp (spv = sv jph(sp)), pit and
// p_n (K1's pit block), the base p, the stage tracer and the base tracer.  sigma-dot is rebuilt top-down from the
// running sum of conv exactly as K4 rebuilds it (conv_acc / sd_of), and each tracer's upper-face flux is carried
// down the column (face_flux_v).  adq, dqs and q_n are the expressions of K4 (pe25d_k4.h) written out again
// textually, on the same factors, in a file built with the same -ffp-contract mode: an fp64 tracer equal to q
// stays equal to q bit for bit.  (fp32: the compiler pairs K4's theta and q chains into packed instructions, which
// round q differently from this kernel's contraction; fp32 tracers are held to the fp32 tolerance.)
#pragma once
#include "pe25d_dev.h"

namespace gcm {

// NC tracers per launch chunk (blockIdx.y = chunk): spu, sv, pit and sigma-dot are loaded and rebuilt once
// per level for all NC of them.  SAME: the stage state is the base state (predictor): no base tracer read.
template <typename T, int NC, bool SAME>
__global__ __launch_bounds__(kTrCols * kTrRows) void pe_tracer_kernel(TracerArgsT<T> a) {
    const Idx ix{a.W, a.H, a.L, a.wrap};
    const int W = a.W, L = a.L;
    // tiles (row group, column tile) in contiguous runs per XCD (workgroups b, b+8, ... share one), column tile
    // fastest: the rows j - 1 / j + 1 a tile reads belong to tiles of the same XCD, close in time (L2 hits)
    const int ncol = (W + kTrCols - 1) / kTrCols;
    const int n0 = a.j1 - a.j0, nrows = n0 + (a.jb1 - a.jb0);
    const int ntiles = ncol * ((nrows + kTrRows - 1) / kTrRows);
    const int per_xcd = (int)(gridDim.x / 8);
    const int tile = (int)(blockIdx.x % 8) * per_xcd + (int)(blockIdx.x / 8);
    if (tile >= ntiles) return;
    const int rg = tile / ncol, ct = tile - rg * ncol;
    const int i = ct * kTrCols + (int)(threadIdx.x % kTrCols);
    // a wave is 64 columns of ONE row: the row and every row offset below are wave-uniform (scalar registers)
    // (r: the row's place in the launch, [j0, j1) then [jb0, jb1))
    const int r = rg * kTrRows + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kTrCols));
    if (i >= W || r >= nrows) return;
    const int j = r < n0 ? a.j0 + r : a.jb0 + (r - n0);
    const int iw = i == 0 ? W - 1 : i - 1, ie = i + 1 == W ? 0 : i + 1;
    const long toff = (long)blockIdx.y * NC * a.tstride;
    const T *c = a.c + toff, *sc = a.sc + toff;
    T *oc = a.oc + toff;
    // every request is a scalar base (field, row, level) + ONE 32-bit byte offset per lane (i, i - 1 or i + 1), as
    // in K4: the base goes through an opaque scalar register pair, else the compiler keeps a 64-bit per-lane address
    // per request and stream (two VGPRs each: 160 VGPRs for four tracers)
    const auto sbase = [](const T *p) {
        unsigned long long v = (unsigned long long)p;
        unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
        asm volatile("" : "+s"(lo), "+s"(hi));
        return (__attribute__((address_space(1))) char *)(((unsigned long long)hi << 32) | lo);
    };
    const unsigned ob_c = (unsigned)i * (unsigned)sizeof(T), ob_w = (unsigned)iw * (unsigned)sizeof(T),
                   ob_e = (unsigned)ie * (unsigned)sizeof(T);
    const auto at = [sbase](const T *base, unsigned ol) { return *(const __attribute__((address_space(1))) T *)(sbase(base) + ol); };

    const int jg_row = wrapi(a.row0 + j, a.Hg);
    const T inv_dxj = a.inv_dxj[jg_row], inv_dy = a.inv_dy, dt = a.dt;
    const T h_dxj = T(0.5) * inv_dxj, h_dy = T(0.5) * inv_dy;
    const long p_n = ix.r2(j - 1), p_c = ix.r2(j), p_s = ix.r2(j + 1);
    const T sp_c = a.sp[p_c + i], sp_s = a.sp[p_s + i], sp_n = a.sp[p_n + i];
    const T jph_c = (sp_c + sp_s) * T(0.5), jph_n = (sp_n + sp_c) * T(0.5);
    const T pb_c = a.p[p_c + i];
    const T inv_pn = rcp(a.pn[p_c + i]);
    const T pit_c = a.pit[p_c + i];
    const long rn = ix.r3(j - 1), rc = ix.r3(j), rs = ix.r3(j + 1);

    // running sum of conv from the top, and per tracer the flux through the upper face of the level
    // (zero at the top of the column: sd wraps to sd[0] = 0) and the stage value of the own cell
    T rc_c = T(0.0);
    T fq_up[NC], sq_c[NC];
#pragma unroll
    for (int n = 0; n < NC; ++n) {
        fq_up[n] = T(0.0);
        sq_c[n] = at(sc + n * a.tstride + rc + (long)(L - 1) * W, ob_c);
    }
#pragma unroll 1
    for (int k = L - 1; k >= 0; --k) {
        const long kc = (long)k * W, km = k > 0 ? kc - W : kc;
        // (the lane offsets are made opaque once per level, so that their use stays next to the requests)
        unsigned oc_, ow_, oe_;
        oc_ = ob_c; ow_ = ob_w; oe_ = ob_e;
        asm volatile("" : "+v"(oc_), "+v"(ow_), "+v"(oe_));
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
        // all requests of the level first: the stores below may alias the base tracer (the corrector writes
        // in place), so a request placed after a store would wait for it
        T sq_e[NC], sq_w[NC], sq_n[NC], sq_s[NC], sq_m[NC], bq_c[NC];
#pragma unroll
        for (int n = 0; n < NC; ++n) {
            const T *s = sc + n * a.tstride;
            sq_e[n] = at(s + rc + kc, oe_); sq_w[n] = at(s + rc + kc, ow_);
            sq_n[n] = at(s + rn + kc, oc_); sq_s[n] = at(s + rs + kc, oc_);
            sq_m[n] = at(s + rc + km, oc_);                      // the level below (k == 0: sd = 0, any finite value)
            bq_c[n] = SAME ? sq_c[n] : at(c + n * a.tstride + rc + kc, oc_);
        }
#pragma unroll
        for (int n = 0; n < NC; ++n) {
            // ---- advec_t, dynamics.py:174-181 (K4's adq)
            const T adq = (spu_c * (sq_c[n] + sq_e[n]) - spu_w * (sq_w[n] + sq_c[n])) * h_dxj +
                          (spv_c * (sq_c[n] + sq_s[n]) - spv_n * (sq_n[n] + sq_c[n])) * h_dy;
            // ---- advec_sig, dynamics.py:49-52 (K4's fq / dqs)
            const T fq = face_flux_v(sq_c[n], sq_m[n], sd_c);
            const T dqs = -((fq - fq_up[n]) * inv_ds);
            fq_up[n] = fq;
            const T q_n = (bq_c[n] * pb_c - (adq + dqs) * dt) * inv_pn;
            *(__attribute__((address_space(1))) T *)(sbase(oc + n * a.tstride + rc + kc) + oc_) = q_n;
            sq_c[n] = sq_m[n];
        }
    }
}

// chunks of nc = 4, 2 or 1 tracers (pe25d_tracers.hip, launch_tracers); instantiated in pe25d_tracer_f{64,32}.hip
template <typename T>
TracerKernel<T> tracer_kernel_for(int nc, bool same) {
    if (nc == 4) return same ? pe_tracer_kernel<T, 4, true> : pe_tracer_kernel<T, 4, false>;
    if (nc == 2) return same ? pe_tracer_kernel<T, 2, true> : pe_tracer_kernel<T, 2, false>;
    return same ? pe_tracer_kernel<T, 1, true> : pe_tracer_kernel<T, 1, false>;
}

}  // namespace gcm

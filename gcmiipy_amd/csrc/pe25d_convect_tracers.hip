// GCM_PE25D, convective mixing of the passive tracers (gcm_set_tracer_convect): every tracer that has opted in is set
// to its mass-weighted mean over each block the convective adjustment pools in the same column at the same moment; one
// launch per application of the adjustment, immediately ahead of it on the same stream.  The contract: include/gcmcore.h.
//
//   per column (level k = 0 is the bottom): the blocks are the adjustment's -- the same p and theta as they stand just
//     ahead of it, the same kappa_c, the same routine convect_push (pe25d_convect.h), no second criterion
//   per merged block (n > 1) over levels [k0, k0 + n) and opted-in tracer c, in float64 for either storage type:
//     D  = dsig[k0];  D  = D  + dsig[k]           k = k0 + 1 .. k0 + n - 1   (convect_block_d)
//     Cs = c[k0] dsig[k0];  Cs = Cs + c[k] dsig[k]   likewise                (convect_block_cs)
//     c[k] <- Cs / D for every level of the block, rounded once to the storage type
//   levels of unmerged blocks, tracers that have not opted in and stable columns are not written.  p is constant in a
//   column: sum_k c p dsig is conserved to rounding.  mix_q plays no part.
//
// The order of the two sums is the contract, and it is NOT the merge-tree order in which the adjustment forms Qs and D
// of a block: a tracer equal to q equals the mixed q to rounding, not to the bit.
//
// Every operation is rounded on its own: contraction is off for the whole file (the Makefile builds it with
// -ffp-contract=fast-honor-pragmas, as pe25d_convect.hip), host and device; the host probe gcm_convect_tracer_columns
// runs the very routines the kernel calls.
//
// The kernel has the adjustment's shape: one wave is one workgroup and 64 consecutive columns i of one row, a lane owns
// the column (j, i), the request of a level is one contiguous run.
//   pass 1, registers only: the adjustment's pass 1, statement for statement.  A wave with no unstable lane returns
//     here, having read p and theta once and written nothing.
//   pass 2: the adjustment's pooling with the block stack in LDS, so that the block lengths are the adjustment's bits;
//     zeros are pushed for q (Qs is not used, and q is not read).  Stable lanes of the wave push and then leave.
//   pass 3, unstable lanes: D of every merged block, formed once, goes to the block's Wt slot (pooling is done: S and Wt
//     are free).  Then per opted-in tracer (their base offsets are a kernel argument) the column is PARKED IN THE
//     STACK'S S ARRAY -- slot k holds c[k], read level by level, kCvBatch requests in flight, each one contiguous run
//     -- and every merged block forms Cs from there and stores the mean.  (The alternative, reading a block's levels
//     from L2 a second time, makes the requests of a level ragged across the lanes; a private array indexed at run time
//     would go to scratch.)
// LDS of a workgroup: the adjustment's, convect_lds_bytes(L); 160 KB hold L = 57 (gcm_set_tracer_convect refuses more).
#pragma clang fp contract(off)
#include "pe25d_convect.h"

namespace gcm {

// ---------------------------------------------------------------- the sums of a merged block (host and device: one routine each)
// levels [k0, k0 + n), sequential, ascending from k0; dsig[k] and c(k) in float64
template <class Ds>
__host__ __device__ inline double convect_block_d(const Ds &dsig, int k0, int n) {
    double D = dsig[k0];
    for (int k = k0 + 1; k < k0 + n; ++k) D = D + dsig[k];
    return D;
}
template <class C, class Ds>
__host__ __device__ inline double convect_block_cs(C &c, const Ds &dsig, int k0, int n) {
    double Cs = c(k0) * dsig[k0];
    for (int k = k0 + 1; k < k0 + n; ++k) Cs = Cs + c(k) * dsig[k];
    return Cs;
}

// gcm_convect_tracer_columns: [ncol][L] columns through convect_push (zeros for q) and the two sums; no handle, no device
int convect_tracer_columns(int ncol, int L, const double *y, const double *w, const double *dsig, const double *c,
                           double *c_out, int32_t *nblk, std::string *err) {
    if (ncol < 0 || L < 1 || (ncol > 0 && (!y || !w || !dsig || !c || !c_out))) {
        *err = "gcm_convect_tracer_columns: ncol must be >= 0, L >= 1; y, w, dsig, c and c_out are required";
        return GCM_ERR_ARG;
    }
    CvHostStack st(L);
    for (int col = 0; col < ncol; ++col) {
        const size_t o = (size_t)col * L;
        int top = 0;
        for (int k = 0; k < L; ++k) top = convect_push(st, top, y[o + k], w[o + k], 0.0, dsig[k]);
        const auto cc = [&](int k) { return c[o + k]; };
        int k = 0;
        for (int b = 0; b < top; ++b) {
            const int n = st.n(b);
            const double mean = n > 1 ? convect_block_cs(cc, dsig, k, n) / convect_block_d(dsig, k, n) : 0.0;
            for (int e = k + n; k < e; ++k) {
                c_out[o + k] = n > 1 ? mean : c[o + k];
                if (nblk) nblk[o + k] = n;
            }
        }
    }
    return GCM_OK;
}

// ---------------------------------------------------------------- the kernel
template <typename T>
struct CvTrArgsT {
    const T *p;                      // [j][i], interior row 0
    const T *t;                      // [j][k][i], interior row 0: theta as it stands ahead of the adjustment
    T *c;                            // tracer 0 of the current set, [j][k][i], row 0
    const double *sig, *dsig;        // [L]
    const double *exner_tab;
    double ptop, kdiff;              // kappa_c - kappa
    int dry;
    int W, L;
    int j0, nrows;                   // the rows of the launch: [j0, j0 + nrows)
    int ntr;                         // the opted-in tracers, and where each starts from c
    long off[GCM_MAX_TRACERS];
};

// the column parked in the stack's S array: slot k holds c[k]
struct CvParked {
    CvLdsStack &st;
    __device__ double operator()(int k) { return st.S(k); }
};

// grid (column blocks of 64, rows)
template <typename T>
__global__ __launch_bounds__(kCvThreads) void pe_convect_tracers_kernel(CvTrArgsT<T> a) {
    extern __shared__ double cvt_lds[];
    const int W = a.W, L = a.L;
    const int lane = threadIdx.x;
    const int i = blockIdx.x * kCvThreads + lane;
    const int r = (int)blockIdx.y;
    if (r >= a.nrows) return;                              // (uniform: the grid has nrows rows)
    const int j = a.j0 + r;
    const bool live = i < W;
    const long c3 = (long)j * L * W + (live ? i : 0);      // (a lane past the row loads nothing, stores nothing)
    const double pc = live ? (double)a.p[(long)j * W + i] : 0.0;

    // ---- pass 1: is any y[k] < y[k - 1]  (pe_convect_kernel's)
    bool unstable = false;
    if (live) {
        double prev = 0.0;
        for (int k = 0; k < L; k += kCvBatch) {
            T th[kCvBatch];
#pragma unroll
            for (int n = 0; n < kCvBatch; ++n)
                if (k + n < L) th[n] = a.t[c3 + (long)(k + n) * W];
#pragma unroll
            for (int n = 0; n < kCvBatch; ++n) {
                const int kk = k + n;
                if (kk < L) {
                    double y = (double)th[n];
                    if (!a.dry) y = y / convect_r(a.sig[kk] * pc + a.ptop, a.kdiff);
                    if (kk > 0 && y < prev) unstable = true;
                    prev = y;
                }
            }
        }
    }
    if (!__any(unstable ? 1 : 0)) return;

    // ---- pass 2: the wave has an unstable lane  (pe_convect_kernel's, with zeros for q)
    double *tab = cvt_lds;
    for (int n = lane; n < kExnerTabDoubles; n += kCvThreads) tab[n] = a.exner_tab[n];
    __syncthreads();
    CvLdsStack st;
    st.base = cvt_lds + kExnerTabDoubles + lane;
    st.cnt = (int *)(cvt_lds + kExnerTabDoubles + (size_t)5 * L * kCvThreads) + lane;
    st.L = L;
    if (!live) return;
    int top = 0;
    for (int k = 0; k < L; k += kCvBatch2) {
        T th[kCvBatch2];
#pragma unroll
        for (int n = 0; n < kCvBatch2; ++n)
            if (k + n < L) th[n] = a.t[c3 + (long)(k + n) * W];
#pragma unroll
        for (int n = 0; n < kCvBatch2; ++n) {
            const int kk = k + n;
            if (kk < L) {
                const double pl = a.sig[kk] * pc + a.ptop;
                const double pi = exner(pl, tab);
                double y = (double)th[n], w;
                if (a.dry) {
                    w = pi * a.dsig[kk];
                } else {
                    const double rr = convect_r(pl, a.kdiff);
                    y = y / rr;
                    w = (pi * rr) * a.dsig[kk];
                }
                top = convect_push(st, top, y, w, 0.0, a.dsig[kk]);
            }
        }
    }
    if (!unstable) return;                                 // a stable lane of an unstable wave: nothing to write

    // ---- pass 3: D of the merged blocks once (into their Wt slots), then tracer by tracer
    {
        int k = 0;
        for (int b = 0; b < top; ++b) {
            const int n = st.n(b);
            if (n > 1) st.Wt(b) = convect_block_d(a.dsig, k, n);
            k += n;
        }
    }
    CvParked parked{st};
    for (int f = 0; f < a.ntr; ++f) {
        T *const c = a.c + a.off[f] + c3;
        for (int k = 0; k < L; k += kCvBatch) {
            T v[kCvBatch];
#pragma unroll
            for (int n = 0; n < kCvBatch; ++n)
                if (k + n < L) v[n] = c[(long)(k + n) * W];
#pragma unroll
            for (int n = 0; n < kCvBatch; ++n)
                if (k + n < L) st.S(k + n) = (double)v[n];
        }
        int k = 0;
        for (int b = 0; b < top; ++b) {
            const int n = st.n(b);
            if (n > 1) {
                const T mean = (T)(convect_block_cs(parked, a.dsig, k, n) / st.Wt(b));
                for (int kk = k; kk < k + n; ++kk) c[(long)kk * W] = mean;
            }
            k += n;
        }
    }
}

// ---------------------------------------------------------------- the handle's side
static void drop_all(Pe25d *m) {
    for (bool &on : m->tr.convect) on = false;
    m->tr.n_convect = 0;
}
// the tracers' storage went (gcm_set_tracers with another count): so do the opt-ins, as the forcing and the mixing do
void tracers_convect_forget(Pe25d *m) { drop_all(m); }

// gcm_set_tracer_convect.  Everything is checked, and the kernel's LDS attribute is in place (the kernel is
// instantiated and launched in this unit alone), before the flag changes: a refused call changes nothing.  The flag is
// read on the host where the next application is queued: nothing in flight depends on it
int pe25d_set_tracer_convect(Pe25d *m, int tracer, bool on, std::string *err) {
    if (!m->wrap) {
        *err = "gcm_set_tracer_convect: latitude bands are not carried yet (single domains only: a band's ghost rows are "
               "adjusted locally, and their tracers would have to be)";
        return GCM_ERR_UNSUPPORTED;
    }
    if (tracer < 0 || tracer >= m->tr.n) {
        *err = "gcm_set_tracer_convect: tracer must be 0 .. gcm_tracer_count - 1";
        return GCM_ERR_ARG;
    }
    if (on && !m->tr.convect_lds) {
        const size_t need = convect_lds_bytes(m->L);
        if (need > kCvLdsCap) {
            *err = "gcm_set_tracer_convect: the block stack of " + std::to_string(m->L) + " levels takes " + std::to_string(need) +
                   " bytes of LDS, a workgroup has " + std::to_string(kCvLdsCap);
            return GCM_ERR_UNSUPPORTED;
        }
        const void *k = m->f32 ? (const void *)pe_convect_tracers_kernel<float> : (const void *)pe_convect_tracers_kernel<double>;
        if (int rc = hip_rc(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need), "gcm_set_tracer_convect", err))
            return rc;
        m->tr.convect_lds = need;
    }
    if (m->tr.convect[tracer] != on) m->tr.n_convect += on ? 1 : -1;
    m->tr.convect[tracer] = on;
    return GCM_OK;
}

int pe25d_tracer_convected(const Pe25d *m, int tracer) {
    if (tracer < 0 || tracer >= m->tr.n) return GCM_ERR_ARG;
    return m->tr.convect[tracer] ? 1 : 0;
}

template <typename T>
static int cvt_launch(Pe25d *m, int set, int j0, int j1, hipStream_t s, std::string *err) {
    PeBufs<T> &B = bufs<T>(m);
    const PeConvect &z = m->convect;
    CvTrArgsT<T> a{};
    a.p = B.st[set][GCM_P]; a.t = B.st[set][GCM_T];
    a.c = (T *)tr_field(m, 0, 0);
    a.sig = m->lev_tab; a.dsig = m->lev_tab + m->L;
    a.exner_tab = m->exner_tab;
    a.ptop = m->cfg.ptop; a.kdiff = z.kappa_c - kKappa;
    a.dry = z.kappa_c == 0.0 ? 1 : 0;
    a.W = m->W; a.L = m->L;
    a.j0 = j0; a.nrows = j1 - j0;
    for (int f = 0; f < m->tr.n; ++f)
        if (m->tr.convect[f]) a.off[a.ntr++] = (long)f * tr_stride(m);
    const dim3 grid((m->W + kCvThreads - 1) / kCvThreads, a.nrows);
    hipLaunchKernelGGL(pe_convect_tracers_kernel<T>, grid, dim3(kCvThreads), m->tr.convect_lds, s, a);
    if (hipGetLastError() != hipSuccess) { *err = "hip: convect tracers kernel launch failed"; return GCM_ERR_HIP; }
    return GCM_OK;
}

// The opted-in tracers' mixing over own rows [j0, j1) of the current tracers, from p and theta of state set `set`, on `s`,
// pe25d_convect_tables in place: pe25d_convect_rows queues it immediately ahead of the adjustment's launch, which
// overwrites the theta it reads.  Nothing is launched, joined or recorded where no tracer has opted in.
// The tracers' stream protocol (pe25d_tracers.hip), hazard 4: the launch writes the current tracers on the caller's
// stream.  Ahead of it `s` joins the last stage's tracer launches on the other streams (transport, mixing, forcing:
// pe25d_join_tracers).  Behind it the next stage's tracer launch on the second stream reads what it wrote: the fork at
// the last K4 is invalidated (pe25d_fork_invalidate, what pe25d_phase_wrote does for a launch that writes u and v), so
// that the next chain B follows the caller's stream's position -- this launch, and the adjustment behind it -- instead
// of the last K4's stop event.  With one stream both are stream order.
int pe25d_convect_tracers_rows(Pe25d *m, int set, int j0, int j1, hipStream_t s, std::string *err) {
    if (m->tr.n_convect <= 0) return GCM_OK;
    j0 = std::clamp(j0, 0, m->H); j1 = std::clamp(j1, j0, m->H);
    if (j1 <= j0) return GCM_OK;
    if (!m->wrap || !m->tr.convect_lds) { *err = "convect tracers: opted in on a handle that cannot take the launch"; return GCM_ERR_STATE; }
    pe25d_join_tracers(m, s);
    if (int rc = m->f32 ? cvt_launch<float>(m, set, j0, j1, s, err) : cvt_launch<double>(m, set, j0, j1, s, err)) return rc;
    pe25d_fork_invalidate(m);
    return GCM_OK;
}

}  // namespace gcm

// GCM_PE25D, convective adjustment (gcm_set_convect, gcm_convect_step): every column's theta, and optionally q, is mixed
// wherever it is statically unstable against a neutral profile, conserving the column's enthalpy and water; one launch
// per step behind the Held-Suarez forcing and the boundary layer and ahead of the moist physics.  The contract: include/gcmcore.h.
//
//   per cell (device, float64 for either storage type, rounded once to it; level k = 0 is the bottom):
//     p_lev = sig[k] p + ptop;  Pi = (p_lev / P0)^kappa (exner());  r = 1 (kappa_c = 0: dry), else
//     r = exp((kappa_c - kappa) log(p_lev / P0));  y = theta / r (dry: theta itself);  w = (Pi r) dsig[k]
//   per column, pool adjacent violators from the bottom up (convect_push, host and device: one routine):
//     k = 0 .. L - 1: push the block (S = w y, Wt = w, Qs = q dsig[k], D = dsig[k], n = 1, value = y); while there is a
//     block below and value < below.value (strict; a NaN compares false) the two become one: S = below.S + S, likewise
//     Wt, Qs, D, n, in that operand order, then value = S / Wt
//     every level of a block with n > 1:  theta <- value r (dry: value);  mix_q: q <- Qs / D.  n = 1: not written
//   per own column: count += 1 where the column had a merged block, levels += sum of n over its merged blocks
//
// Both loops are bounded by L: a push merges at most the blocks there are.  This is the weighted isotonic regression
// of y, the exact limit of the pairwise adjustment: no iteration count, no tolerance.  sum_k y w = sum_k T dsig and
// sum_k q dsig are conserved to rounding.
//
// Every operation is rounded on its own: contraction is off for the whole file (the Makefile builds it with
// -ffp-contract=fast-honor-pragmas), host and device, so that a column gets the same bits whichever launch -- a single
// domain's, a band's own rows', a neighbour's ghost rows' -- produces it, and the host probe gcm_convect_columns runs
// the very routine the kernel calls.
//
// The state's layout is [j][k][i]: one lane owns the column (j, i), a workgroup is one wave, 64 consecutive i of one
// row, so the request of a level is one contiguous run.
//   pass 1, registers only: the column is marched kCvBatch levels at a time; y and a running "some y[k] < y[k - 1]".
//     A column has a merged block iff that holds.  Most columns are stable at most steps: a wave with no unstable lane
//     returns here (__any), having read p and theta once, and written nothing.
//   pass 2, waves with an unstable lane: the column is marched again (its lines are still in L2), now with q, Pi and w,
//     and pooled with the block stack in LDS, slot-major ([slot][lane]: a wave's access to a slot is 64 consecutive
//     words, conflict-free).  A runtime-indexed private array would go to scratch.  Stable lanes of the wave pool too
//     (they only push) and write nothing.  The Exner table is loaded into LDS here, not before: pass 1 needs none.
// LDS of a workgroup: the 2 KB Exner table and 44 bytes per level and lane (five doubles and a count), sized from L at
// launch: 69.6 KB at L = 24 (two workgroups share a CU), 112 KB at L = 40, 160 KB hold L = 57.
#pragma clang fp contract(off)
#include "pe25d_convect.h"

namespace gcm {

// (the pooling routine convect_push, convect_r and the host's stack: pe25d_convect.h, shared with pe25d_convect_tracers.hip)
int convect_check(const gcm_convect *cv, const char *fn, std::string *err) {
    const auto bad = [&](const char *what) { *err = std::string(fn) + ": " + what; return GCM_ERR_ARG; };
    if (!cv) return bad("no parameters");
    if (!std::isfinite(cv->kappa_c) || !(cv->kappa_c >= 0.0 && cv->kappa_c < 1.0)) return bad("kappa_c must be finite and lie in [0, 1)");
    if (cv->mix_q != 0 && cv->mix_q != 1) return bad("mix_q must be 0 or 1");
    return GCM_OK;
}

// gcm_convect_columns: [ncol][L] columns of the compared value through convect_push; no handle, no device
int convect_columns(int ncol, int L, const double *y, const double *w, const double *q, const double *dsig, int mix_q,
                    double *y_out, double *q_out, int32_t *nblock, std::string *err) {
    if (ncol < 0 || L < 1 || (mix_q != 0 && mix_q != 1) || (ncol > 0 && (!y || !w || !q || !dsig))) {
        *err = "gcm_convect_columns: ncol must be >= 0, L >= 1, mix_q 0 or 1; y, w, q and dsig are required";
        return GCM_ERR_ARG;
    }
    CvHostStack st(L);
    for (int c = 0; c < ncol; ++c) {
        const size_t o = (size_t)c * L;
        int top = 0;
        for (int k = 0; k < L; ++k) top = convect_push(st, top, y[o + k], w[o + k], q[o + k], dsig[k]);
        int k = 0;
        for (int b = 0; b < top; ++b) {
            const int n = st.n(b);
            for (int e = k + n; k < e; ++k) {
                if (y_out) y_out[o + k] = n > 1 ? st.val(b) : y[o + k];
                if (q_out) q_out[o + k] = n > 1 && mix_q ? st.Qs(b) / st.D(b) : q[o + k];
                if (nblock) nblock[o + k] = n;
            }
        }
    }
    return GCM_OK;
}

// ---------------------------------------------------------------- the kernel
// (the constants of the kernel's shape and the lane's stack in LDS, CvLdsStack: pe25d_convect.h)
size_t convect_lds_bytes(int L) { return sizeof(double) * kExnerTabDoubles + kCvSlotBytes * (size_t)L * kCvThreads; }

template <typename T>
struct CvArgsT {
    const T *p;                      // [j][i], interior row 0
    T *t, *q;                        // [j][k][i], interior row 0
    const double *sig, *dsig;        // [L]
    const double *exner_tab;
    double *count, *levels;          // [H][W] own rows, or null: the launch accumulates nothing
    double ptop, kdiff;              // kappa_c - kappa
    int dry, mix_q;
    int W, L, H;
    int j0, n0, jb0, nrows;          // the rows of the launch: [j0, j0 + n0), then from jb0 on (a band's ghost rows: negative / >= H)
};

// grid (column blocks of 64, rows)
template <typename T>
__global__ __launch_bounds__(kCvThreads) void pe_convect_kernel(CvArgsT<T> a) {
    extern __shared__ double cv_lds[];
    const int W = a.W, L = a.L;
    const int lane = threadIdx.x;
    const int i = blockIdx.x * kCvThreads + lane;
    const int r = (int)blockIdx.y;
    if (r >= a.nrows) return;                              // (uniform: the grid has nrows rows)
    const int j = r < a.n0 ? a.j0 + r : a.jb0 + (r - a.n0);
    const bool live = i < W;
    const long c3 = (long)j * L * W + (live ? i : 0);      // (a lane past the row loads nothing, stores nothing)
    const double pc = live ? (double)a.p[(long)j * W + i] : 0.0;

    // ---- pass 1: is any y[k] < y[k - 1]
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

    // ---- pass 2: the wave has an unstable lane
    double *tab = cv_lds;
    for (int n = lane; n < kExnerTabDoubles; n += kCvThreads) tab[n] = a.exner_tab[n];
    __syncthreads();
    CvLdsStack st;
    st.base = cv_lds + kExnerTabDoubles + lane;
    st.cnt = (int *)(cv_lds + kExnerTabDoubles + (size_t)5 * L * kCvThreads) + lane;
    st.L = L;
    if (!live) return;
    int top = 0;
    for (int k = 0; k < L; k += kCvBatch2) {
        T th[kCvBatch2], qq[kCvBatch2];
#pragma unroll
        for (int n = 0; n < kCvBatch2; ++n)
            if (k + n < L) {
                const long o = c3 + (long)(k + n) * W;
                th[n] = a.t[o];
                qq[n] = a.q[o];
            }
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
                top = convect_push(st, top, y, w, (double)qq[n], a.dsig[kk]);
            }
        }
    }
    if (!unstable) return;                                 // a stable lane of an unstable wave: nothing to write
    double levels = 0.0;
    int k = 0;
    for (int b = 0; b < top; ++b) {
        const int n = st.n(b);
        if (n > 1) {
            const double val = st.val(b);
            const double qm = a.mix_q ? st.Qs(b) / st.D(b) : 0.0;
            for (int kk = k; kk < k + n; ++kk) {
                const long o = c3 + (long)kk * W;
                double theta = val;
                if (!a.dry) theta = val * convect_r(a.sig[kk] * pc + a.ptop, a.kdiff);
                a.t[o] = (T)theta;
                if (a.mix_q) a.q[o] = (T)qm;
            }
            levels = levels + (double)n;
        }
        k += n;
    }
    if (a.count && j >= 0 && j < a.H) {
        const long o2 = (long)j * W + i;
        a.count[o2] = a.count[o2] + 1.0;
        a.levels[o2] = a.levels[o2] + levels;
    }
}

// ---------------------------------------------------------------- the handle's side
// the wave's stack at the handle's L must fit a workgroup's LDS (160 KB); the kernel's dynamic LDS size is set once, here (the
// kernel is instantiated and launched in this unit alone)
int pe25d_convect_fits(Pe25d *m, const char *fn, std::string *err) {
    PeConvect &z = m->convect;
    if (z.lds_bytes) return GCM_OK;
    const size_t need = convect_lds_bytes(m->L), cap = kCvLdsCap;
    if (need > cap) {
        *err = std::string(fn) + ": the block stack of " + std::to_string(m->L) + " levels takes " + std::to_string(need) +
               " bytes of LDS, a workgroup has " + std::to_string(cap);
        return GCM_ERR_UNSUPPORTED;
    }
    const void *k = m->f32 ? (const void *)pe_convect_kernel<float> : (const void *)pe_convect_kernel<double>;
    if (int rc = hip_rc(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need), fn, err)) return rc;
    z.lds_bytes = need;
    return GCM_OK;
}

// the launches' level tables (pe25d_level_table) and the parameters of the launches that follow; dt:
// what an accumulating launch adds to the seconds (the step's dt; 0 for gcm_convect_step, which takes none)
int pe25d_convect_tables(Pe25d *m, const gcm_convect *cv, double dt, std::string *err) {
    if (int rc = convect_check(cv, "convect", err)) return rc;
    if (!std::isfinite(dt)) { *err = "convect: dt must be finite"; return GCM_ERR_ARG; }
    if (int rc = pe25d_convect_fits(m, "convect", err)) return rc;
    if (!pe25d_level_table(m, "convect", err)) return GCM_ERR_HIP;
    PeConvect &z = m->convect;
    z.kappa_c = cv->kappa_c;
    z.mix_q = cv->mix_q;
    z.dt = dt;
    return GCM_OK;
}

template <typename T>
static int cv_launch(Pe25d *m, int set, int j0, int j1, int jb0, int jb1, bool accumulate, hipStream_t s, std::string *err) {
    PeBufs<T> &B = bufs<T>(m);
    const PeConvect &z = m->convect;
    CvArgsT<T> a{};
    a.p = B.st[set][GCM_P]; a.t = B.st[set][GCM_T]; a.q = B.st[set][GCM_Q];
    a.sig = m->lev_tab; a.dsig = m->lev_tab + m->L;
    a.exner_tab = m->exner_tab;
    a.count = accumulate ? z.sums.acc : nullptr;
    a.levels = accumulate ? z.sums.acc + (size_t)m->H * m->W : nullptr;
    a.ptop = m->cfg.ptop; a.kdiff = z.kappa_c - kKappa;
    a.dry = z.kappa_c == 0.0 ? 1 : 0; a.mix_q = z.mix_q;
    a.W = m->W; a.L = m->L; a.H = m->H;
    a.j0 = j0; a.n0 = std::max(0, j1 - j0); a.jb0 = jb0; a.nrows = a.n0 + std::max(0, jb1 - jb0);
    const dim3 grid((m->W + kCvThreads - 1) / kCvThreads, a.nrows);
    hipLaunchKernelGGL(pe_convect_kernel<T>, grid, dim3(kCvThreads), z.lds_bytes, s, a);
    if (hipGetLastError() != hipSuccess) { *err = "hip: convect kernel launch failed"; return GCM_ERR_HIP; }
    return GCM_OK;
}

// rows [j0, j1) and [jb0, jb1) of state set `set` (-1: the current one) on `s`, pe25d_convect_tables in place.
// accumulate: the own rows' counts are added to the registered sums, and the call counts as one application
int pe25d_convect_rows(Pe25d *m, int set, int j0, int j1, int jb0, int jb1, bool keep_ghosts, bool accumulate, hipStream_t s,
                       std::string *err) {
    PeConvect &z = m->convect;
    if (!m->lev_tab || !z.lds_bytes) { *err = "convect: no tables in place"; return GCM_ERR_STATE; }
    if (accumulate && !z.sums.acc) { *err = "convect: no sums to accumulate into (gcm_set_convect)"; return GCM_ERR_STATE; }
    if (set < 0) set = m->cur_i;
    if (std::max(0, j1 - j0) + std::max(0, jb1 - jb0) <= 0) return GCM_OK;
    // the opted-in tracers are mixed in this application's blocks, from theta as it stands: immediately ahead, in stream
    // order (single domains: the own rows are [j0, j1); without an opt-in nothing is queued)
    if (int rc = pe25d_convect_tracers_rows(m, set, j0, j1, s, err)) return rc;
    pe25d_phase_wrote(m, set, keep_ghosts, false);         // the launch writes theta and q and reads p, theta and q
    if (int rc = m->f32 ? cv_launch<float>(m, set, j0, j1, jb0, jb1, accumulate, s, err)
                        : cv_launch<double>(m, set, j0, j1, jb0, jb1, accumulate, s, err))
        return rc;
    if (accumulate) sums_count(z.sums, z.dt);
    return GCM_OK;
}

}  // namespace gcm

// GCM_PE25D: 2.5-D sigma-level primitive equations, Matsuno on the lat-lon C-grid
// (reference dynamics.py:15-237, low_pass.py:41-78, temperature.py:7-19).
//
// Device layout: 3-D fields are [j][k][i] (i fastest, then the L levels, then the rows), so a
// latitude band and its ghost rows are contiguous slabs; p is [j][i].  The host-facing layout
// stays the reference's [k][j][i]; set/get transpose on the device.
//
// One half_timestep (dynamics.py:183-227) is five launches on two streams:
//   K1  spu_filter  spu = arakawa_1977(su * iph(sp))            one workgroup per (row, level pair)
//   K2b pit         conv, pit, p_n (sigma-dot is rebuilt in K4)  one thread per (j, i) column
//   K2a geopot      rho, phi                                     one thread per (j, i) column
//   K3  pgf_filter  pgfu = arakawa_1977(pgu + phiu)              one workgroup per (row, level pair)
//   K4  update      advec_m_pu, advec_sig, advec_t, un_pu/un_pv  one thread per (j, i) column
// K1 -> K2b and K2a -> K3 are independent chains (two streams), K4 needs both.
// The zonal filter is a complex Stockham FFT in LDS: two levels of one row are packed as
// real and imaginary part (the filter multiplier is real and symmetric in the wavenumber, so
// it acts on both parts independently), multiplied by S[j][n] and transformed back.
//
// This unit: the column kernels K2 and the stage orchestration that launches K1 .. K4 (half_t and its steps) -- whatever
// records or waits for the stage's events, or sets a protocol flag to anything but "invalid".  The handle's life cycle
// and data movement: pe25d_state.hip; grey radiation: pe25d_physics.hip; diagnostics and taps: pe25d_diag.hip.
#include "pe25d_host.h"

#include <hip/hip_ext.h>

namespace gcm {

// ---------------------------------------------------------------- K2: column kernels
// K2a pe_geopot_kernel: rho, phi from the stage theta and surface pressure (compute_geopotential);
// K2b pe_pit_kernel: pit = sum_k conv and p_n from the filtered mass flux (aflux).  They are two
// kernels because they sit on two independent chains, K1 -> K2b and K2a -> K3 (see half_t).
// The per-level stp that phi needs after the column sum is parked in LDS, park[k][thread],
// instead of a round trip through HBM.  (kColThreads: pe25d_dev.h)
// sum_k dsig[k] u[k] and sum_k dsig[k] v[k] of one column, k = L-1 .. 0 with cs_acc, as K4 accumulates them.  Eight levels of
// BOTH fields are requested at a time, then added in order: one memory latency per eight levels (a load per iteration
// waits one per level: 20 us for the two ghost rows of a band, on the edge rows' chain; round 4: the two fields together)
template <typename T>
__device__ __forceinline__ void column_sum2(const T *cu, const T *cv, const T *dsig, int L, int W, T *su, T *sv) {
    T au = T(0.0), av = T(0.0);
    int k = L - 1;
    for (; k >= 7; k -= 8) {
        T x[8], y[8];
#pragma unroll
        for (int n = 0; n < 8; ++n) { x[n] = cu[(long)(k - n) * W]; y[n] = cv[(long)(k - n) * W]; }
#pragma unroll
        for (int n = 0; n < 8; ++n) { au = cs_acc(au, x[n], dsig[k - n]); av = cs_acc(av, y[n], dsig[k - n]); }
    }
    for (; k >= 0; --k) { au = cs_acc(au, cu[(long)k * W], dsig[k]); av = cs_acc(av, cv[(long)k * W], dsig[k]); }
    *su = au; *sv = av;
}
// LMAX > 0: L <= LMAX and the per-level stp stay in registers (loops unrolled over LMAX; no LDS
// park, so the occupancy is not limited by it); LMAX == 0: any L, stp parked in LDS
// CS: the launch also forms the column sums of its rows (a band's ghost rows; a template parameter, because the
// mere presence of that code in the kernel cost the plain instantiation 40 % of its speed)
// (Round 4, priced with a timing proxy and not built: this kernel also emitting pgu + phiu of every level, so that K3
// becomes a pure filter -- K2a 74.8 -> 116 us, K3 171 -> the 120 us K1 takes for the same traffic: -1.2 % of the step,
// profiles/r04/ab_k2a_emits_pgu_phiu_proxy.txt.)
template <typename T, int LMAX = 0, bool CS = false>
__global__ __launch_bounds__(kColThreads) void pe_geopot_kernel(PeArgsT<T> a) {
    __shared__ double tab[kExnerTabDoubles];
    extern __shared__ unsigned char park_raw[];
    T *park = (T *)park_raw;                    // [L][kColThreads] (LMAX == 0)
    T stp_reg[LMAX > 0 ? LMAX : 1];
    for (int n = threadIdx.x; n < kExnerTabDoubles; n += kColThreads) tab[n] = a.exner_tab[n];
    __syncthreads();
    const Idx ix{a.W, a.H, a.L, a.wrap};
    const int W = a.W, L = a.L;
    // tiles (row, column block) in contiguous runs of rows per XCD, as pe_update_kernel
    const int iblocks = (W + kColThreads - 1) / kColThreads;
    const int per_xcd = gridDim.x / 8;
    const int tile = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
    const int jrel = tile / iblocks;
    const int na = a.j1 - a.j0;
    if (jrel >= na + (a.jb1 - a.jb0)) return;
    const int i = (tile - jrel * iblocks) * kColThreads + threadIdx.x;
    const int j = jrel < na ? a.j0 + jrel : a.jb0 + (jrel - na);
    if (i >= W) return;
    if (CS) {
        // a band's ghost rows in one launch: their column sums too (see pe_colsum_kernel)
        T cs_u, cs_v;
        column_sum2(a.su + ix.r3(j) + i, a.sv + ix.r3(j) + i, a.dsig, L, W, &cs_u, &cs_v);
        a.scs_u[ix.r2(j) + i] = cs_u;
        a.scs_v[ix.r2(j) + i] = cs_v;
    }
    if (j < a.geo_j0 || j >= a.geo_j1) return;
    T *pk = park + threadIdx.x;
    const int jg = wrapi(a.row0 + j, a.Hg);
    const T spc = a.sp[ix.r2(j) + i];
    const long c3 = ix.r3(j);
    // ---- compute_geopotential, dynamics.py:111-143
    const T hmG = a.heightmap ? a.heightmap[(long)jg * W + i] * T(kG) : T(0.0) * T(kG);
    // LMAX > 0: the whole theta column is requested before any of it is used (one HBM latency per
    // column instead of one per level)
    T tcol[LMAX > 0 ? LMAX : 1];
    if (LMAX > 0) {
#pragma unroll
        for (int k = 0; k < LMAX; ++k) tcol[k] = k < L ? a.st[c3 + (long)k * W + i] : T(0.0);
    }
    T t_k = LMAX > 0 ? tcol[0] : a.st[c3 + i];
    T ex_k = exner(spc * a.sig[0] + a.ptop, tab);
    const T t0 = t_k, ex0 = ex_k;                       // level 0, for the k wrap at the top
    T acc = T(0.0);
    constexpr int kUnrollA = LMAX > 0 ? LMAX : 6, kUnrollB = LMAX > 0 ? LMAX : 1;
#pragma unroll kUnrollA
    for (int k = 0; k < (LMAX > 0 ? LMAX : L); ++k) {
        if (LMAX > 0 && k >= L) break;
        const T tp = spc * a.sig[k] + a.ptop;
        T t_n, ex_n;
        if (k + 1 < L) {
            t_n = LMAX > 0 ? tcol[k + 1 < LMAX ? k + 1 : 0] : a.st[c3 + (long)(k + 1) * W + i];
            ex_n = exner(spc * a.sig[k + 1] + a.ptop, tab);
        } else {
            t_n = t0;            // kp() wraps to the bottom layer, coordinates_3d.py:55-56
            ex_n = ex0;
        }
        const T rho = rho_of(tp, t_k, ex_k);            // tp / (Rd t / (P0/tp)**kappa)
        const T s1 = (a.sig[k] * spc * rcp(rho)) * a.dsig[k];
        const T stp = stp_of(t_k, t_n, ex_k, ex_n);
        const T s2 = a.sigt[k] * stp;
        acc += s1 - s2;
        if (LMAX > 0) stp_reg[k] = stp;
        else pk[k * kColThreads] = stp;
        t_k = t_n;
        ex_k = ex_n;
    }
    T run = acc + hmG;                                  // stp_n[0], dynamics.py:132
    a.phi[c3 + i] = run;
#pragma unroll kUnrollB
    for (int k = 1; k < (LMAX > 0 ? LMAX : L); ++k) {        // phi = cumsum(stp_n), stp_n = km(stp)
        if (LMAX > 0 && k >= L) break;
        run = add_rn(run, LMAX > 0 ? stp_reg[k - 1] : pk[(k - 1) * kColThreads]);
        if ((k & 1) == 0) a.phi[c3 + (long)k * W + i] = run;     // anchors: even levels only
    }
}

// aflux, dynamics.py:35-46: pit = sum_k conv (ascending, as np.sum over the outer axis) and
// p_n = p - pit dt (dynamics.py:194).  sigma-dot itself is not materialised: the update kernel
// rebuilds it on the fly from pit.
template <typename T>
__global__ __launch_bounds__(256) void pe_pit_kernel(PeArgsT<T> a) {
    const Idx ix{a.W, a.H, a.L, a.wrap};
    const int W = a.W, L = a.L;
    const int iblocks = (W + 255) / 256;
    const int per_xcd = gridDim.x / 8;
    const int tile = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
    const int jrel = tile / iblocks;
    if (jrel >= a.j1 - a.j0) return;
    const int i = (tile - jrel * iblocks) * 256 + threadIdx.x;
    const int j = a.j0 + jrel;
    if (i >= W) return;
    const int iw = i == 0 ? W - 1 : i - 1;
    const int jg = wrapi(a.row0 + j, a.Hg);
    const T inv_dxj = a.inv_dxj[jg], inv_dy = a.inv_dy;
    const T spc = a.sp[ix.r2(j) + i], spn = a.sp[ix.r2(j - 1) + i], sps = a.sp[ix.r2(j + 1) + i];
    const T jph_c = (spc + sps) * T(0.5), jph_n = (spn + spc) * T(0.5);  // jph(sp) at j, j-1
    const long c3 = ix.r3(j), n3 = ix.r3(j - 1);
    T pit = T(0.0);
#pragma unroll 12
    for (int k = 0; k < L; ++k) {
        const long o = c3 + (long)k * W;
        const T spv_c = a.sv[o + i] * jph_c;
        const T spv_n = a.sv[n3 + (long)k * W + i] * jph_n;
        pit += ((a.spu[o + i] - a.spu[o + iw]) * inv_dxj + (spv_c - spv_n) * inv_dy) * a.dsig[k];
    }
    a.pit[ix.r2(j) + i] = pit;
    a.pn[ix.r2(j) + i] = a.p[ix.r2(j) + i] - pit * a.dt;
    if (a.nseg > 1) {
        // top-down partial sums at the segment boundaries, exactly as pe_update_kernel accumulates
        T rc = T(0.0);
        int s = a.nseg - 2;
        int stop = seg_lo(s + 1, a.nseg, L);
#pragma unroll 4
        for (int k = L - 1; k >= 1 && s >= 0; --k) {
            const long o = c3 + (long)k * W;
            rc = conv_acc(rc, a.spu[o + i], a.spu[o + iw], inv_dxj, a.sv[o + i], jph_c, a.sv[n3 + (long)k * W + i], jph_n,
                          inv_dy, a.dsig[k]);
            if (k == stop) {
                a.part[(long)s * a.part_stride + ix.r2(j) + i] = rc;
                --s;
                if (s >= 0) stop = seg_lo(s + 1, a.nseg, L);
            }
        }
    }
}

// The partial sums of conv at the segment boundaries alone (pit itself comes from pe_pit2d_kernel),
// rows [j0, j1) and [jb0, jb1): a band's edge rows, which K4 marches in level segments so that they
// are done -- and on their way to the neighbours -- long before the interior rows (a K4 workgroup
// is a chain of L dependent levels, however few rows it has).  Same accumulation as pe_pit_kernel.
template <typename T>
__global__ __launch_bounds__(256) void pe_part_kernel(PeArgsT<T> a) {
    const Idx ix{a.W, a.H, a.L, a.wrap};
    const int W = a.W, L = a.L;
    const int iblocks = (W + 255) / 256;
    const int jrel = blockIdx.x / iblocks;
    const int i = (blockIdx.x - jrel * iblocks) * 256 + threadIdx.x;
    const int na = a.j1 - a.j0;
    if (i >= W || jrel >= na + (a.jb1 - a.jb0)) return;
    const int j = jrel < na ? a.j0 + jrel : a.jb0 + (jrel - na);
    const int iw = i == 0 ? W - 1 : i - 1;
    const int jg = wrapi(a.row0 + j, a.Hg);
    const T inv_dxj = a.inv_dxj[jg], inv_dy = a.inv_dy;
    const T spc = a.sp[ix.r2(j) + i], spn = a.sp[ix.r2(j - 1) + i], sps = a.sp[ix.r2(j + 1) + i];
    const T jph_c = (spc + sps) * T(0.5), jph_n = (spn + spc) * T(0.5);
    const long c3 = ix.r3(j), n3 = ix.r3(j - 1);
    T rc = T(0.0);
    int s = a.nseg - 2;
    int stop = seg_lo(s + 1, a.nseg, L);
    // the levels of one segment are requested together, then accumulated in order
    for (int k = L - 1; s >= 0;) {
        constexpr int kB = 8;
        T xu[kB], xw[kB], xv[kB], xn[kB];
        const int n = min(kB, k - stop + 1);
#pragma unroll
        for (int m = 0; m < kB; ++m) {
            const long o = (long)max(k - m, stop) * W;
            xu[m] = a.spu[c3 + o + i]; xw[m] = a.spu[c3 + o + iw]; xv[m] = a.sv[c3 + o + i]; xn[m] = a.sv[n3 + o + i];
        }
#pragma unroll
        for (int m = 0; m < kB; ++m)
            if (m < n) rc = conv_acc(rc, xu[m], xw[m], inv_dxj, xv[m], jph_c, xn[m], jph_n, inv_dy, a.dsig[k - m]);
        k -= n;
        if (k < stop) {
            a.part[(long)s * a.part_stride + ix.r2(j) + i] = rc;
            --s;
            if (s >= 0) stop = seg_lo(s + 1, a.nseg, L);
        }
    }
}

// U, V of the stage state's rows [j0, j1) and [jb0, jb1): the rows no K4 has produced them for (a
// state that came through gcm_set_state; a band's ghost rows, which the exchange fills)
template <typename T>
__global__ __launch_bounds__(256) void pe_colsum_kernel(PeArgsT<T> a) {
    const Idx ix{a.W, a.H, a.L, a.wrap};
    const int W = a.W;
    const int iblocks = (W + 255) / 256;
    const int jrel = blockIdx.x / iblocks;
    const int i = (blockIdx.x - jrel * iblocks) * 256 + threadIdx.x;
    const int na = a.j1 - a.j0;
    if (i >= W || jrel >= na + (a.jb1 - a.jb0)) return;
    const int j = jrel < na ? a.j0 + jrel : a.jb0 + (jrel - na);
    T cs_u, cs_v;
    column_sum2(a.su + ix.r3(j) + i, a.sv + ix.r3(j) + i, a.dsig, a.L, W, &cs_u, &cs_v);
    a.scs_u[ix.r2(j) + i] = cs_u;
    a.scs_v[ix.r2(j) + i] = cs_v;
}

static bool async_edges(const Pe25d *m) { return m->send_buf[0] && m->send_buf[1]; }

// ================================================================== host side: the stage
// (the handle, struct Pe25d, and the helpers shared with the other host units: pe25d_host.h)

// pe25d_create: the dynamic LDS sizes of the kernels a stage launches
template <typename T>
static bool stage_lds_attributes_t(const Pe25d *m) {
    const int L = m->L;
    if ((spu_filter_loop_kernel_for<T>(m->cplan) &&
         hipFuncSetAttribute((const void *)spu_filter_loop_kernel_for<T>(m->cplan), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)filter_loop_lds_bytes<T>(m)) != hipSuccess) ||
        hipFuncSetAttribute((const void *)spu_filter_kernel_for<T>(m->cplan), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)filter_lds_bytes<T>(m)) != hipSuccess ||
        hipFuncSetAttribute((const void *)pgf_filter_kernel_for<T>(m->cplan), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)filter_lds_bytes<T>(m)) != hipSuccess ||
        hipFuncSetAttribute((const void *)pit2d_kernel_for<T>(m->cplan), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)pit2d_lds_bytes<T>(m)) != hipSuccess ||
        hipFuncSetAttribute((const void *)pe_geopot_kernel<T, 0>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(L * kColThreads * sizeof(T))) != hipSuccess ||
        hipFuncSetAttribute((const void *)pe_geopot_kernel<T, 0, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(L * kColThreads * sizeof(T))) != hipSuccess)
        return false;
    for (const int R : {7, 3})                   // K4: rows per workgroup x (same, oddtop)
        for (const int v : {0, 1, 2, 3})
            if (hipFuncSetAttribute((const void *)update_rows_kernel_for<T>(R, v & 1, v & 2), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)upd_lds_bytes<T>(R, L)) != hipSuccess)
                return false;
    return true;
}
bool stage_lds_attributes(const Pe25d *m) { return m->f32 ? stage_lds_attributes_t<float>(m) : stage_lds_attributes_t<double>(m); }

static void tick(Pe25d *m, hipStream_t s) {
    if (m->ev && m->ev_used && *m->ev_used < m->ev->size()) (void)hipEventRecord((*m->ev)[(*m->ev_used)++], s);
}

// What follows a kernel launch: nothing, or the event `ev` (see Pe25d::stop_events).  stop_only: K4's ev_k4, signalled as
// the kernel's stop event or not at all, never by a record
struct Then { hipEvent_t ev = nullptr; bool stop_only = false; };

// The one way a stage launches a kernel that an event follows: `kern` on `st`, and `then.ev` behind it -- the kernel's
// own completion with stop events, else a record behind the launch (none for `stop_only`: without stop events
// k4_fork_valid stays false and nobody waits for ev_k4).
template <typename... P>
static void launch(const Pe25d *m, void (*kern)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, Then then, const P &...args) {
    if (then.ev && m->stop_events) return hipExtLaunchKernelGGL(kern, grid, block, (unsigned)lds, st, nullptr, then.ev, 0, args...);
    hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
    if (then.ev && !then.stop_only) (void)hipEventRecord(then.ev, st);
}

// `a` over rows [j0, j1) and [jb0, jb1)
template <typename T>
static PeArgsT<T> rows_of(PeArgsT<T> a, int j0, int j1, int jb0 = 0, int jb1 = 0) { a.j0 = j0; a.j1 = j1; a.jb0 = jb0; a.jb1 = jb1; return a; }

// pe_geopot_kernel over the rows of `c` ([j0, j1) and [jb0, jb1)); c.geo_j0 / geo_j1: the rows it forms phi
// for, c.cs_rows: it also forms the column sums of all its rows
template <typename T>
static void launch_geopot(const Pe25d *m, const PeArgsT<T> &c, hipStream_t st) {
    const int rows = (c.j1 - c.j0) + (c.jb1 - c.jb0), L = m->L;
    if (rows <= 0) return;
    const long tiles = (long)((m->W + kColThreads - 1) / kColThreads) * rows;
    const size_t park = L <= 40 ? 0 : sizeof(T) * (size_t)L * kColThreads;
    void (*kern)(PeArgsT<T>) =
        c.cs_rows ? (L <= 24 ? pe_geopot_kernel<T, 24, true> : L <= 40 ? pe_geopot_kernel<T, 40, true> : pe_geopot_kernel<T, 0, true>)
                  : (L <= 24 ? pe_geopot_kernel<T, 24> : L <= 40 ? pe_geopot_kernel<T, 40> : pe_geopot_kernel<T, 0>);
    launch(m, kern, dim3((unsigned)((tiles + 7) / 8 * 8)), dim3(kColThreads), park, st, Then{}, c);
}

// Column sums and geopotential anchors of the stage state's rows that no kernel of the previous stage left:
// all rows' sums of a freshly set state, else a band's two ghost rows next to its own (pit of row j takes V of
// row j - 1; the intermediates extend to row j1) -- and, in the same launch, the geopotential of a band's south
// ghost row (K4 of row j1 - 1 takes phi of row j1).  `a`: the stage's arguments.
template <typename T>
static void prep_rows(Pe25d *m, const PeArgsT<T> &a, int stage_set, bool p2, int j1, int ext, hipStream_t sb) {
    PeArgsT<T> c = a;
    c.jb0 = c.jb1 = 0;
    bool fresh = false;
    if (!p2) { c.j0 = j1; c.j1 = j1 + ext; }
    else if (!m->cs_valid[stage_set]) {
        c.j0 = m->wrap ? 0 : -1;
        c.j1 = m->H + ext;
        m->cs_valid[stage_set] = true;
        fresh = true;
    } else if (m->nseg_edge > 1 && m->edge_cs_set != stage_set) {   // + the own edge rows (marched in segments: no sums from K4)
        c.j0 = -1; c.j1 = kGhost;
        c.jb0 = m->H - kGhost; c.jb1 = m->H + 1;
    } else {
        c.j0 = -1; c.j1 = 0;
        c.jb0 = m->H; c.jb1 = m->H + 1;
    }
    c.cs_rows = p2 ? 1 : 0;
    c.geo_j0 = j1; c.geo_j1 = j1 + ext;
    if (fresh && (c.j1 - c.j0) > 8) {
        // a whole state's sums: the plain column-sum kernel (no thermodynamics compiled in), then the ghost row
        hipLaunchKernelGGL(pe_colsum_kernel<T>, dim3((unsigned)((m->W + 255) / 256) * (c.j1 - c.j0)), dim3(256), 0, sb, c);
        c.cs_rows = 0;
        c.j0 = j1; c.j1 = j1 + ext;
    }
    if (!m->wrap || (fresh && c.cs_rows)) launch_geopot(m, c, sb);
}

// ---------------------------------------------------------------- one Euler stage
// One Euler stage over rows [j0, j1): state `stage_set` -> `out_set`, base = current.
// mode 0: everything; mode 1: K1-K3 on all rows + K4 on the two edge rows of either side (the rows
// a neighbouring band needs); mode 2: K4 on the remaining interior rows.  Modes 1 + 2 == mode 0.
// chained: the call comes from gcm_band_run's own sequence (nothing but the stage's kernels between two stages on `s`)
// Two chains on two streams (a cross-queue dependency costs ~10 us on this chip when the waiting queue
// is already idle, ~3 us when the event completed earlier: tools/micro/sync_cost.hip):
//   A, the caller's stream:  K2a (own rows) -> K3 -> K4 (all rows, or the interior rows of a band)
//   B, the second stream:    column sums and anchors of the ghost rows -> K1 (+ pit) [-> a band's edge
//                            rows: their partial sums, K4, pack; the exchange and the unpack follow]
// A is the long chain and runs without waiting for anything that has not long finished: K4 waits for
// B's K1 (done while K3 runs), the next stage's K2a for B's edge rows (done while the interior rows
// run).  A never touches ghost rows, so it never waits for an exchange; B does, in stream order.
// (Round 4, built and rejected: the edge rows' K3 as a launch of its own on chain B right behind K2a, so that their
// K4, the pack and the exchange start before the interior rows' K4 takes the chip.  Four rows are 48 workgroups of
// five dependent LDS passes: 30-60 us on a chain that already holds K1's ghost-row launch and the partial sums, and
// the N = 8 band got 4 % slower with no exchange time and 10 % slower with 40 us of it
// (profiles/r04/ab_band_edge_k3_on_chain_b.txt: `base` = with it).)
// Stage: what a stage is, decided once from the handle's state as it begins (stage_facts); the steps read it, change only the handle.
template <typename T>
struct Stage {
    int stage_set, out_set, j0, j1, mode; double dt;
    PeArgsT<T> a;                                // the stage's arguments; every launch takes its own rows (rows_of)
    hipStream_t s;                               // chain A: the caller's stream
    hipStream_t sb;                              // chain B: the second stream (the caller's when the handle has one stream)
    hipStream_t se;                              // the edge rows' stream (mode 1): chain B's with send buffers registered, else the caller's
    hipEvent_t fork;                             // what chain B follows on the caller's stream (chain_b_head)
    int ext;                                     // intermediates are also needed on row j1 (south)
    bool p2;                                     // pit from the 2-D column sums (pe_pit2d_kernel) where K4 marches whole columns and can leave them
    bool split;                                  // modes 1 + 2 of a band with interior rows between its edge rows
    bool edge_segs;                              // the edge rows are marched in level segments (update_edges)
    FilterLoopKernel<T> k1;                      // the looping form of K1, or null
    bool tr_prev;                                // the last stage's tracer launch on another stream may still run (hazard 1, chain_b_head)
    bool ghosts_queued;                          // the ghost rows' column sums and anchors are queued behind the unpack already
    bool split_k1;                               // K1 of the own rows on the third stream, of the ghost-dependent rows on the second
};

template <typename T>
static Stage<T> stage_facts(Pe25d *m, int stage_set, int out_set, double dt, int j0, int j1, hipStream_t s, int mode, bool chained) {
    Stage<T> g{};
    g.stage_set = stage_set; g.out_set = out_set; g.j0 = j0; g.j1 = j1; g.mode = mode; g.dt = dt;
    g.a = make_args<T>(m, stage_set, out_set, dt);
    g.ext = m->wrap ? 0 : 1;
    g.p2 = m->pit2d && g.a.nseg == 1;
    if (g.p2) { g.a.ocs_u = bufs<T>(m).cs[out_set][0]; g.a.ocs_v = bufs<T>(m).cs[out_set][1]; }     // (the column sums K4 leaves)
    g.s = s; g.sb = m->aux ? m->aux : s;
    g.se = (mode == 1 && async_edges(m) && m->aux) ? m->aux : s;
    // the previous stage's K4 (its own completion, ev_k4, when nothing else that B reads or overwrites was queued
    // since: k4_fork_valid, which only stop events set), else the stream's position now
    g.fork = (m->k4_fork_valid && chained) ? m->ev_k4 : m->ev_fork;
    g.split = mode != 0 && (j1 - j0) > 2 * kGhost;
    g.edge_segs = g.split && g.p2 && m->nseg_edge > 1;
    if (mode == 2) return g;                     // (K4 of the interior rows: the rest belongs to modes 0 and 1)
    g.k1 = (m->cfg.filter && m->W > 1 && !m->filter_no_loop) ? spu_filter_loop_kernel_for<T>(m->cplan) : nullptr;
    g.tr_prev = last_tracers_in_flight(m);
    g.ghosts_queued = m->ghost_ready == stage_set && (!g.p2 || m->cs_valid[stage_set]);
    // A band inside gcm_band_run (the ghost rows' column sums and anchors are queued behind the unpack already):
    // K1 is row-local -- spu of row j takes su and sp of row j only, pit of row j the column sums of rows j - 1, j
    // and sp of rows j - 1 .. j + 1 -- so the band's OWN rows need nothing from the exchange.  They go to a third
    // stream that waits for the previous stage's K4 only (spu of rows [0, H), pit of rows [2, H - 2]: what the
    // interior rows' K4 reads), and the second stream keeps the launch for the rows that do need ghost data (spu of
    // the south ghost row, pit of rows 0, 1, H - 1, H).  The interior rows' K4 then waits for the own-row launch
    // alone, not for the exchange chain (round 3: 32 us per corrector stage of the N = 8 band of C4).
    g.split_k1 = g.k1 && mode == 1 && m->aux2 && g.p2 && g.ghosts_queued && (j1 - j0) >= 2 * kGhost + 3 &&
                 (m->nseg_edge == 1 || m->edge_cs_set == stage_set);
    return g;
}

// ---- chain B: everything that reads the whole stage state, ghost rows included.  Its head: what it waits for, and the ghost rows
template <typename T>
static void chain_b_head(Pe25d *m, const Stage<T> &g) {
    if (m->aux) {
        if (g.fork == m->ev_fork) (void)hipEventRecord(m->ev_fork, g.s);
        (void)hipStreamWaitEvent(m->aux, g.fork, 0);
    }
    // hazard 1 of a band's tracers: this stage's K1 overwrites spu, pit and p_n -- and its K4 the state sets -- that
    // the last stage's tracer launch on another stream may still read (ev_tr_int, see stage_tracers): chain B waits for
    // it here, and so does the caller's stream where it takes the edge rows (no send buffers: the tracers' edge rows
    // read what that launch wrote); the third stream's K1 follows it in stream order, or waits for it in chain_b_k1_pit.
    // At the van Leer scheme's reach of two rows (gcm_set_band_tracer_rows(2)) the same wait covers what is new: the
    // edge launch of this stage writes the out set's rows 0, 1, H - 2, H - 1, which the last stage's interior launch
    // (rows [2, H - 2)) read as its stage set at j -+ 2 -- at reach one it read rows 1 and H - 2 of them -- and it
    // reads rows 2, 3, H - 4, H - 3, which that launch wrote (at reach one: rows 2 and H - 3).  The other direction:
    // this stage's interior launch reads the stage set's rows 0, 1, H - 2, H - 1, which the LAST stage's edge launch
    // wrote on the edge rows' stream (at reach one: rows 1 and H - 2, of the same launch).  It waits for ev_a, and
    // ev_a follows that launch on every path: K1 of all rows is queued on chain B behind it (send buffers: the same
    // stream; none: chain B's fork follows the caller's stream, which carried it), and the split K1's own rows on the
    // third stream wait for the fork and for ev_edges, recorded behind the pack that follows it
    if (g.tr_prev) {
        follow_last_tracers(m, g.sb);
        if (g.mode == 1 && g.se != g.sb) follow_last_tracers(m, g.se);
    }
    if (g.ghosts_queued) m->ghost_ready = -1;                    // queued behind the unpack already
    else prep_rows<T>(m, g.a, g.stage_set, g.p2, g.j1, g.ext, g.sb);
    // (the own edge rows' column sums of this state were queued on the third stream behind the edge rows' K4
    // of the stage that produced it: everything on the second stream that reads them waits for that)
    if (m->aux2 && m->edge_cs_set == g.stage_set) (void)hipStreamWaitEvent(g.sb, m->ev_cs, 0);
}

// The looping K1 over `rows` rows of `c`: all pairs of a row in one workgroup when there are rows enough to fill the
// chip, else groups; with `pit` (the 2-D form of pit) one more workgroup per row forms pit and p_n (pe_pit2d_row)
template <typename T>
static void launch_k1(const Pe25d *m, FilterLoopKernel<T> k1, const PeArgsT<T> &c, int rows, bool pit, hipStream_t st, hipEvent_t ev) {
    const StageK1 k = stage_k1_launch(m->L, rows, m->cus);      // (pe25d_stage_geometry.h)
    launch(m, k1, dim3(rows, k.ny + (pit ? 1 : 0)), dim3(m->cplan.ok ? m->cplan.threads : kFftThreads), filter_loop_lds_bytes<T>(m), st,
           Then{ev}, c, k.ppw, pit ? k.ny : -1);
}

// ---- chain B: K1 and pit of rows [j0, j1 + ext), and ev_a behind them (what K4 of the interior rows takes from this chain)
template <typename T>
static void chain_b_k1_pit(Pe25d *m, const Stage<T> &g) {
    const int j0 = g.j0, j1 = g.j1, ext = g.ext;
    const PeArgsT<T> a = rows_of(g.a, j0, j1 + ext);
    const int fft_threads = m->cplan.ok ? m->cplan.threads : kFftThreads;
    bool pit_done = false, ev_a_done = false;
    if (g.split_k1) {                            // (see stage_facts)
        (void)hipStreamWaitEvent(m->aux2, g.fork, 0);
        // (the previous stage's edge rows: su, sp of rows 0, 1, H - 2, H - 1 -- and its tracers' edge rows, queued
        // ahead of the pack: they read spu, pit and p_n of those rows, which this K1 overwrites)
        if (m->edges_ev_valid) (void)hipStreamWaitEvent(m->aux2, m->ev_edges, 0);
        if (g.tr_prev) follow_last_tracers(m, m->aux2);
        PeArgsT<T> c = rows_of(a, j0, j1);
        c.pit_j0 = j0 + kGhost; c.pit_j1 = j1 - kGhost + 1;
        launch_k1<T>(m, g.k1, c, j1 - j0, true, m->aux2, m->ev_a);             // (ev_a: what K4 of the interior rows takes)
        c = rows_of(a, j0, j0 + kGhost, j1 - 1, j1 + ext);
        c.spu_j0 = j1; c.spu_j1 = j1 + ext;
        launch_k1<T>(m, g.k1, c, kGhost + 1 + ext, true, g.sb, nullptr);
        pit_done = ev_a_done = true;             // (chain B waits for ev_a in update_edges, ahead of the edge rows' partial sums)
    } else if (g.k1) {
        ev_a_done = g.p2 && m->aux;              // pit rides in the launch: ev_a follows K1 itself
        launch_k1<T>(m, g.k1, a, a.j1 - a.j0, g.p2, g.sb, ev_a_done ? m->ev_a : nullptr);
        pit_done = g.p2;
    } else {
        hipLaunchKernelGGL(spu_filter_kernel_for<T>(m->cplan), dim3(a.j1 - a.j0, (m->L + 1) / 2), dim3(fft_threads), filter_lds_bytes<T>(m), g.sb, a);
    }
    if (g.p2 && !pit_done) {
        hipLaunchKernelGGL(pit2d_kernel_for<T>(m->cplan), dim3(a.j1 - a.j0), dim3(fft_threads), pit2d_lds_bytes<T>(m), g.sb, a);
    } else if (!g.p2) {
        const long tiles = (long)((m->W + 255) / 256) * (a.j1 - a.j0);
        hipLaunchKernelGGL(pe_pit_kernel<T>, dim3((unsigned)((tiles + 7) / 8 * 8)), dim3(256), 0, g.sb, a);
    }
    if (m->aux && !ev_a_done) (void)hipEventRecord(m->ev_a, m->aux);      // (behind the pit kernel)
}

// ---- the passive tracers that do not belong to a band's edge rows (those: update_edges)
template <typename T>
static void stage_tracers(Pe25d *m, const Stage<T> &g) {
    if (m->tr.n <= 0) return;
    // Single domain: on chain B right behind K1 + pit and after ev_a, so that K4 on
    //      chain A never waits for them and they run beside K2a, K3 and K4.  Two invariants hold them in place:
    //      * the next stage's K1 must not overwrite spu, pit or p_n while this launch still reads them: it is
    //        queued on this same stream behind it.  (Not on `s` behind K4: chain B forks at ev_k4 when
    //        k4_fork_valid is set, and the next K1 would then race the tracer kernel.)  The state sets it reads
    //        (sp, sv, p) are overwritten only by a later K4, which waits for a later ev_a: behind this launch too;
    //      * everything that returns to the caller joins chain B's tail: gcm_step (and so gcm_time_steps'
    //        stop event), gcm_half_step, gcm_get_tracers, gcm_set_tracers and gcm_sync make `s` wait for ev_tr,
    //        recorded on `aux` behind the last tracer launch (pe25d_join_tracers).
    //      Without tracers nothing is launched, recorded or waited for here.
    //      A band: the whole stage (mode 0) takes the same launch over its own rows, and the next stage's chain B
    //      waits for it on the streams where it does not follow in stream order (ev_tr_int, hazard 1 in chain_b_head).
    if (g.mode == 0) {
        launch_tracers<T>(m, g.a, g.stage_set, g.out_set, g.sb, g.j0, g.j1);
        if (!m->wrap && m->aux) stage_tracers_launched(m, g.sb, false);
    }
    // ---- a band's split stage (modes 1 + 2): the tracers' edge rows go ahead of the pack (see update_edges), the
    //      interior rows [j0 + 2, j1 - 2) here, on the third stream right behind the own rows' K1 (ev_a): off the
    //      exchange chain, which never waits for them within the stage, and beside K2a and K3 on the caller's
    //      stream, whose LDS-bound passes leave memory bandwidth free.  ev_tr_int follows them: the next stage's
    //      chain B waits for it (hazard 1), the caller's stream joins it (pe25d_join_tracers).  Without a third
    //      stream they go to the caller's stream, where the next stage's chain B follows them through the fork.
    if (g.mode == 1 && g.split) {
        hipStream_t ti = m->aux2 ? m->aux2 : g.s;
        if (m->aux && !(g.split_k1 && ti == m->aux2)) (void)hipStreamWaitEvent(ti, m->ev_a, 0);   // (K1 + pit of all rows)
        launch_tracers<T>(m, g.a, g.stage_set, g.out_set, ti, g.j0 + kGhost, g.j1 - kGhost);
        if (ti != g.s) stage_tracers_launched(m, ti, true);
    }
}

// ---- chain A: geopotential of the own rows, then the filtered pressure-gradient force; then the wait for chain B's ev_a
template <typename T>
static void chain_a(Pe25d *m, const Stage<T> &g) {
    const PeArgsT<T> a = rows_of(g.a, g.j0, g.j1);
    PeArgsT<T> c = a;
    c.cs_rows = 0;
    c.geo_j0 = g.j0; c.geo_j1 = g.j1;
    launch_geopot(m, c, g.s);
    // (a looping form of this filter, as K1's, was built and is 25 % SLOWER: its requests and the
    // per-column thermodynamics push it to 187 VGPRs, two waves per SIMD instead of four)
    // (launched with whole waves -- 192 threads for the 144 butterflies of a 1440 row, so that the
    // per-column thermodynamics ahead of the transform fills its lanes -- it takes the same time)
    const bool join = m->aux && g.mode == 1 && async_edges(m);                     // the edge rows' K4 on B takes pgfu
    launch(m, pgf_filter_kernel_for<T>(m->cplan), dim3((unsigned)(8 * ((a.j1 - a.j0 + 7) / 8) * ((m->L + 1) / 2))),
           dim3(m->cplan.ok ? m->cplan.threads : kFftThreads), filter_lds_bytes<T>(m), g.s, Then{join ? m->ev_join : nullptr}, a);
    if (m->aux) (void)hipStreamWaitEvent(g.s, m->ev_a, 0);                         // K4 on A takes spu, pit (and a band's ghost anchors)
}

// K4 over rows [r0, r1) and [rb0, rb1) of `a`, one launch; k4_done: ev_k4 where the launch is the caller's stream's last of the stage
template <typename T>
static void update_rows(const Pe25d *m, PeArgsT<T> a, int r0, int r1, int rb0, int rb1, hipStream_t st, hipEvent_t k4_done = nullptr) {
    const int rows = std::max(0, r1 - r0) + std::max(0, rb1 - rb0);
    if (rows <= 0) return;
    a = rows_of(a, r0, std::max(r0, r1), rb0, std::max(rb0, rb1));
    const int Rg = m->upd_rows, L = m->L;
    // 8 XCDs x (row group, segment) pairs per XCD x column tiles (see the kernel's index map; pe25d_stage_geometry.h)
    const long groups = stage_k4_groups(r1 - r0, rb1 - rb0, Rg);
    const dim3 gg((unsigned)stage_k4_grid(groups, a.nseg, m->W));
    const bool same = a.u == a.su;
    // whole columns of an even number of levels start on an odd level: the geopotential anchor is requested with the
    // even levels only (an odd level steps up from the anchor in the tile below and never reads its own): one request
    // in eleven (seven) less every other level, C4 1.881 -> 1.857 ms per step (round 4, A/B on one box)
    const bool oddtop = stage_k4_oddtop(m->k4_oddtop, a.nseg, L);
    launch(m, update_rows_kernel_for<T>(Rg, same, oddtop), gg, dim3(64 * (Rg + 1)), upd_lds_bytes<T>(Rg, L), st, Then{k4_done, true}, a);
}

// mode 0 -- chain A: K4 of all rows
template <typename T>
static void update_whole(Pe25d *m, const Stage<T> &g) {
    tick(m, g.s);
    update_rows<T>(m, g.a, g.j0, g.j1, 0, 0, g.s, m->ev_k4);
    m->k4_fork_valid = m->stop_events && !(m->ev && m->ev_used);       // (timing runs put records behind the kernel)
    tick(m, g.s);
}

// mode 1 -- the rows the neighbours wait for (an unsplittable, tiny band: all of them).  With send
// buffers registered they are updated and packed on the second stream (chain B), which waits
// for K3 here; the caller's stream goes straight on to the interior rows (mode 2), so the
// two launches share the chip.
template <typename T>
static void update_edges(Pe25d *m, const Stage<T> &g) {
    const int j0 = g.j0, j1 = g.j1;
    const bool as = async_edges(m);
    hipStream_t se = g.se;
    if (g.split_k1) (void)hipStreamWaitEvent(se, m->ev_a, 0);      // the edge rows' partial sums and K4 take spu of own rows
    if (g.edge_segs) {
        // a band's edge rows are marched in level segments (below): the partial sums of conv they start from,
        // behind K1 on chain B and ahead of its wait for K3 (beside the interior rows' K4 this kernel took 50 us
        // instead of 14)
        PeArgsT<T> c = rows_of(g.a, j0, j0 + kGhost + 1, j1 - kGhost, j1 + 1);   // (K4 of row j also takes the sums of row j + 1)
        c.nseg = m->nseg_edge;
        hipLaunchKernelGGL(pe_part_kernel<T>, dim3((unsigned)((m->W + 255) / 256) * (2 * kGhost + 2)), dim3(256), 0, se, c);
    }
    if (m->tr.n > 0) {
        // the tracers' edge rows (the rows a neighbour takes, and the rows next to them), on the stream of the edge
        // rows' K4, behind K1, pit and ev_a and ahead of the wait for K3: they fill chain B's wait.  Hazard 2: in
        // the corrector they read the star tracers' ghost rows, which the post-predictor unpack filled ahead of K1
        // on this stream (gcm_band_run), or on the caller's stream before this call (host-driven exchange).
        // With two ghost rows a side (gcm_set_band_tracer_rows) that unpack fills both from the one segment per
        // tracer, so its completion covers rows -2, -1, H and H + 1 alike; these rows [0, 2) and [H - 2, H) are the
        // only ones whose j -+ 2 leaves the band (the interior launch of stage_tracers reaches own rows 0 and H - 1 at
        // most), and they are exactly the rows the pack below takes at that depth.  A band too short to split
        // (H <= 4) takes the one launch here, behind the same unpack.
        if (g.split) launch_tracers<T>(m, g.a, g.stage_set, g.out_set, se, j0, j0 + kGhost, j1 - kGhost, j1);
        else launch_tracers<T>(m, g.a, g.stage_set, g.out_set, se, j0, j1);
    }
    if (as && m->aux) (void)hipStreamWaitEvent(m->aux, m->ev_join, 0);      // the edge rows' K4 takes pgfu
    if (as && m->aux && m->edges_first && g.split) {
        (void)hipEventRecord(m->ev_pre_edge, se);          // chain B is about to launch the edge rows' K4
        m->pre_edge_pending = true;
    }
    if (g.edge_segs) {
        // the edge rows in level segments: a quarter of the chain of dependent levels, so the pack
        // and the exchange start while the interior rows are still at work
        // (the partial sums of conv they start from: pe_part_kernel, queued behind K1 above)
        PeArgsT<T> c = g.a;
        c.nseg = m->nseg_edge;
        c.ocs_u = c.ocs_v = nullptr;
        update_rows<T>(m, c, j0, j0 + kGhost, j1 - kGhost, j1, se);
    } else if (g.split) {
        update_rows<T>(m, g.a, j0, j0 + kGhost, j1 - kGhost, j1, se);
    } else {
        update_rows<T>(m, g.a, j0, j1, 0, 0, se);
    }
    if (!as) return;
    // (hazard 3: the pack of the new state's edge rows follows the corrector's tracer edge launch above in
    // stream order on `se`; a pack the caller queues -- gcm_halo_pack -- follows `aux` through halo_run)
    SegCopy c{};
    std::string err;
    (void)pe25d_halo_segments(m, true, 0, m->send_buf[0], &c, &err);
    (void)pe25d_halo_segments(m, true, 1, m->send_buf[1], &c, &err);
    launch_seg_copy(c, se, m->stop_events ? m->ev_edges : nullptr);
    if (!m->stop_events) (void)hipEventRecord(m->ev_edges, se);
    m->edges_pending = true;
    m->edges_ev_valid = true;
    if (m->aux2 && g.edge_segs) {
        // the edge rows were marched in level segments and left no column sums: formed here, on the third
        // stream, as soon as the rows exist -- beside the interior rows still at work, off every chain of the
        // next stage (which read them: pit of rows 0 .. 2 and H - 2 .. H)
        (void)hipStreamWaitEvent(m->aux2, m->ev_edges, 0);
        const PeArgsT<T> cc = rows_of(make_args<T>(m, g.out_set, g.out_set, g.dt), j0, j0 + kGhost, j1 - kGhost, j1);
        launch(m, pe_colsum_kernel<T>, dim3((unsigned)((m->W + 255) / 256) * (2 * kGhost)), dim3(256), 0, m->aux2, Then{m->ev_cs}, cc);
        m->edge_cs_set = g.out_set;
    }
}

// mode 2 -- chain A: K4 of the interior rows
template <typename T>
static void update_interior(Pe25d *m, const Stage<T> &g) {
    if (g.split) {
        if (m->pre_edge_pending) (void)hipStreamWaitEvent(g.s, m->ev_pre_edge, 0);
        m->pre_edge_pending = false;
        update_rows<T>(m, g.a, g.j0 + kGhost, g.j1 - kGhost, 0, 0, g.s, m->ev_k4);
        m->k4_fork_valid = m->stop_events;
    }
    // whatever follows on the caller's stream also follows the edge rows
    if (async_edges(m) && m->edges_pending) (void)hipStreamWaitEvent(g.s, m->ev_edges, 0);
    m->edges_pending = false;
}

// The stage, step by step (s = the caller's stream, aux / aux2 = the second / third stream; -> E: E follows the kernel):
//   chain_b_head    aux   waits ev_k4 or ev_fork (s), ev_tr_int, ev_cs;  the ghost rows' column sums and anchors
//   chain_b_k1_pit  aux   K1 + pit -> ev_a                  split K1: aux2 waits the fork, ev_edges, ev_tr_int; own rows' K1 -> ev_a;
//                                                            aux keeps the ghost-dependent rows' K1
//   stage_tracers   aux   mode 0, behind K1 -> ev_tr_int    mode 1: interior rows on aux2 (else s), waits ev_a -> ev_tr_int
//   chain_a         s     K2a, K3 -> ev_join (mode 1 with send buffers); then s waits ev_a
//   update_whole    s     K4 -> ev_k4
//   update_edges    aux (s without send buffers)  waits ev_a (split K1);  partial sums, tracers' edge rows;  waits ev_join;
//                         -> ev_pre_edge;  K4 of the edge rows;  pack -> ev_edges;  aux2 waits ev_edges: column sums -> ev_cs
//   update_interior s     waits ev_pre_edge;  K4 -> ev_k4;  waits ev_edges
template <typename T>
static void half_t(Pe25d *m, int stage_set, int out_set, double dt, int j0, int j1, hipStream_t s, int mode, bool chained) {
    if (j1 <= j0) return;
    const Stage<T> g = stage_facts<T>(m, stage_set, out_set, dt, j0, j1, s, mode, chained);
    m->last_stage_set = stage_set;
    if (mode != 2) {
        chain_b_head(m, g);
        chain_b_k1_pit(m, g);
        stage_tracers(m, g);
        chain_a(m, g);
    }
    m->cs_valid[out_set] = g.p2;                 // (modes 1 + 2 together cover the rows)
    if (mode == 0) update_whole(m, g);
    else if (mode == 1) update_edges(m, g);
    else update_interior(m, g);
}

static void half(Pe25d *m, int stage_set, int out_set, double dt, int j0, int j1, hipStream_t s, int mode = 0, bool chained = false) {
    // (a single domain's stages follow one another on `s` with nothing between them that chain B must wait for)
    const bool ch = chained || (mode == 0 && m->wrap);
    if (m->f32) half_t<float>(m, stage_set, out_set, dt, j0, j1, s, mode, ch);
    else half_t<double>(m, stage_set, out_set, dt, j0, j1, s, mode, ch);
}

// gcm_pe25d_stage_plan: what the steps above launch, by the rules of stage_facts, chain_b_k1_pit, update_whole, update_edges
// and update_interior and with the numbers of pe25d_stage_geometry.h that launch_k1 and update_rows take themselves
int pe25d_stage_plan(const Pe25d *m, int *out, int nout) {
    if (!out || nout < GCM_STAGE_PLAN_WORDS) return GCM_ERR_ARG;
    for (int n = 0; n < GCM_STAGE_PLAN_WORDS; ++n) out[n] = 0;
    const int H = m->H, W = m->W, L = m->L, ext = m->wrap ? 0 : 1;
    const bool p2 = m->pit2d && m->nseg == 1;                                    // (stage_facts)
    const bool loop = m->cfg.filter && W > 1 && !m->filter_no_loop;
    stage_words_k1(out, m->cplan, loop, L, H + ext, m->cus, p2);                 // mode 0: K1 of rows [0, H + ext)
    stage_words_k4(out, W, H, L, m->upd_rows, m->nseg, m->k4_oddtop);
    if (m->wrap || H <= 2 * kGhost) return GCM_OK;                               // (no band, or one too short to split)
    out[GCM_STAGE_BAND] = 1;
    // the split K1 (inside gcm_band_run, the ghost rows' sums queued behind the unpack): its own-rows launch
    if (out[GCM_STAGE_K1_LOOP] && m->aux2 && p2 && H >= 2 * kGhost + 3) {
        const StageK1 k = stage_k1_launch(L, H, m->cus);
        out[GCM_STAGE_K1_SPLIT] = 1;
        out[GCM_STAGE_K1_OWN_WGS_PER_ROW] = k.ny;
        out[GCM_STAGE_K1_OWN_PAIRS_PER_WG] = k.ppw;
        out[GCM_STAGE_K1_OWN_PAIRS_LAST_WG] = k.pairs - (k.ny - 1) * k.ppw;
    }
    const int nseg_edge = (p2 && m->nseg_edge > 1) ? m->nseg_edge : m->nseg;     // (edge_segs)
    out[GCM_STAGE_NSEG_EDGE] = nseg_edge;
    stage_words_k4_launch(out + GCM_STAGE_K4_EDGE_GROUPS, W, kGhost, kGhost, L, m->upd_rows, nseg_edge, m->k4_oddtop);
    stage_words_k4_launch(out + GCM_STAGE_K4_INT_GROUPS, W, H - 2 * kGhost, 0, L, m->upd_rows, m->nseg, m->k4_oddtop);
    return GCM_OK;
}

// gcm_band_run, right behind the unpack on the second stream: the ghost rows that have just arrived belong to
// the state the NEXT stage reads; their column sums and the south ghost row's geopotential depend on nothing
// else, so they are queued here -- beside the interior rows' K4 of the stage still running -- instead of at the
// head of the next stage's chain B, where they were 17 us in front of K1.
int pe25d_prep_ghost_rows(Pe25d *m, std::string *err) {
    if (m->wrap || !m->aux) return GCM_OK;
    int set = m->star_valid ? 2 : m->cur_i;                      // the set the unpack has just filled (pe25d_halo_segments)
    if (m->pack_set >= 0 && m->pack_set != 2) set = m->pack_set;
    if (set != m->last_unpack_set) {
        // the two functions pick the set by the same rule; if they ever disagree the next stage would take its
        // ghost rows' column sums and anchors from rows nobody filled
        *err = "gcm_band_run: the ghost rows just unpacked are not those of the state the next stage reads";
        return GCM_ERR_STATE;
    }
    const bool p2 = m->pit2d && m->nseg == 1;
    if (p2 && !m->cs_valid[set]) return GCM_OK;                  // (a fresh state: the stage does all rows itself)
    if (m->f32) prep_rows<float>(m, make_args<float>(m, set, set, 0.0), set, p2, m->H, 1, m->aux);      // (it picks its rows itself)
    else prep_rows<double>(m, make_args<double>(m, set, set, 0.0), set, p2, m->H, 1, m->aux);
    m->ghost_ready = set;
    return GCM_OK;
}

// The two stages of a Matsuno step by their state sets: the predictor (stage 0) takes the current set to set 2 (star),
// the corrector (stage 1) set 2 to the other of sets 0 / 1, which finish_stage makes the current one.
struct StageSets { int stage_set, out_set; };
static StageSets stage_sets(const Pe25d *m, int stage) { return stage == 0 ? StageSets{m->cur_i, 2} : StageSets{2, 1 - m->cur_i}; }
// phased: gcm_step_phase published the set gcm_halo_pack reads (pack_set) for the stage's duration
static void finish_stage(Pe25d *m, int stage, bool phased = false) {
    m->star_valid = stage == 0;
    if (stage == 0) return;
    m->cur_i = 1 - m->cur_i;
    if (phased) m->pack_set = -1;
}
static int launch_status(std::string *err) {
    if (hipGetLastError() == hipSuccess) return GCM_OK;
    *err = "hip: pe25d kernel launch failed";
    return GCM_ERR_HIP;
}

int pe25d_half(Pe25d *m, int stage, double dt, hipStream_t s, std::string *err) {
    if (!m->wrap) {
        *err = "half_step on a latitude band: use step_part";
        return GCM_ERR_UNSUPPORTED;
    }
    if (stage != 0 && !m->star_valid) {
        *err = "half_step(1) before half_step(0)";
        return GCM_ERR_STATE;
    }
    const StageSets z = stage_sets(m, stage != 0);
    half(m, z.stage_set, z.out_set, dt, 0, m->H, s);
    finish_stage(m, stage != 0);
    pe25d_join_tracers(m, s);
    return launch_status(err);
}

int pe25d_step(Pe25d *m, double dt, hipStream_t s, std::string *err) {
    if (!m->wrap) {
        *err = "gcm_step: a latitude band needs ghost-row exchanges inside the step (use step_part)";
        return GCM_ERR_STATE;
    }
    for (int stage = 0; stage < 2; ++stage) {
        const StageSets z = stage_sets(m, stage);
        half(m, z.stage_set, z.out_set, dt, 0, m->H, s);
        finish_stage(m, stage);
    }
    return launch_status(err);
}

// Latitude band: part 0 = predictor (needs ghost rows of the current state),
// part 1 = corrector (needs ghost rows of the predicted state), then the swap.
int pe25d_step_part(Pe25d *m, int part, double dt, hipStream_t s, std::string *err) {
    if (m->wrap) {
        *err = "step_part: handle is not a latitude band";
        return GCM_ERR_STATE;
    }
    const StageSets z = stage_sets(m, part != 0);
    half(m, z.stage_set, z.out_set, dt, 0, m->H, s);
    finish_stage(m, part != 0);
    return launch_status(err);
}

// Latitude band with the exchange hidden behind the interior rows of K4 (gcm_step_phase):
//   phase 0  predictor K1-K3 + K4 edge rows   -> the predicted edge rows can be sent
//   phase 1  predictor K4 interior rows
//   phase 2  corrector K1-K3 + K4 edge rows   -> the new state's edge rows can be sent
//   phase 3  corrector K4 interior rows, then the swap
// gcm_halo_pack after phase 0 / 2 packs the rows just produced; gcm_halo_unpack after phase 1 / 3
// fills the ghost rows of the predicted / the new current state.
int pe25d_step_phase(Pe25d *m, int phase, double dt, hipStream_t s, std::string *err, bool chained) {
    if (m->wrap) {
        *err = "step_phase: handle is not a latitude band";
        return GCM_ERR_STATE;
    }
    if (phase < 0 || phase > 3) {
        *err = "step_phase: phase must be 0..3";
        return GCM_ERR_ARG;
    }
    const int stage = phase / 2;
    const bool edges = phase % 2 == 0;
    const StageSets z = stage_sets(m, stage);
    if (edges) {                                 // the pack at the end of the edge rows reads the set this stage writes
        m->pack_set = z.out_set;
        if (stage == 0) m->star_valid = true;
    }
    half(m, z.stage_set, z.out_set, dt, 0, m->H, s, edges ? 1 : 2, chained);
    if (!edges) finish_stage(m, stage, true);
    return launch_status(err);
}

// gcm_band_run's one join: whatever follows on `s` also follows what the third stream still holds (the own edge
// rows' column sums of the last stage)
void pe25d_join_third_stream(Pe25d *m, hipStream_t s) {
    if (!m->aux2) return;
    (void)hipEventRecord(m->ev_cs, m->aux2);
    (void)hipStreamWaitEvent(s, m->ev_cs, 0);
}

int pe25d_wait_edges(Pe25d *m, hipStream_t s, std::string *err) {
    if (!async_edges(m)) {
        *err = "wait_edges: no send buffers registered (gcm_set_halo_buffers)";
        return GCM_ERR_STATE;
    }
    if (hipStreamWaitEvent(s, m->ev_edges, 0) != hipSuccess) {
        *err = "hip: wait_edges failed";
        return GCM_ERR_HIP;
    }
    return GCM_OK;
}

}  // namespace gcm

// The kernels of the 2-D shallow-water family and their launchers, templated on the real type T of the
// state and of the arithmetic.  Included by exactly two translation units: sw2d_kernels.hip instantiates
// T = double, sw2d_kernels_f32.hip T = float (GCM_F32 handles), so that each compiles on its own.
//
// Two variants of the same arithmetic (gcm_math.h):
//   staged  one thread per cell, one launch per Euler stage, neighbours through L1/L2;
//           the predicted ("star") state is materialised in HBM.
//   fused   one wave marches down a 60-column strip keeping a 3-row window of the
//           base state and of the predicted state in registers; i+-1 neighbours come
//           from wave64 DPP shifts; predictor and corrector (and both tracer passes)
//           run in one launch, so every field is read once and written once per step.
// The Exner table stays float64 for either T (gcm_math.h exner()).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "gcm_math.h"
#include "sw2d_kernels.h"

namespace gcm {

__device__ __forceinline__ long row_off(int j, int H, int W, bool wrap) {
    if (wrap) {
        j %= H;
        if (j < 0) j += H;
    }
    return (long)j * W;
}

// Member m of an ensemble handle: every field pointer moved to that member's slab.  m is uniform
// over a workgroup (a block index), so the offsets live in scalar registers.
template <typename T>
__device__ __forceinline__ Sw2dArgsT<T> member_args(const Sw2dArgsT<T> &a0, int m) {
    Sw2dArgsT<T> a = a0;
    const long o = (long)m * a0.mstride;
    auto mv = [o](auto *p) { return p ? p + o : p; };
    a.bu = mv(a.bu); a.bv = mv(a.bv); a.bp = mv(a.bp); a.bt = mv(a.bt); a.bq = mv(a.bq);
    a.su = mv(a.su); a.sv = mv(a.sv); a.sp = mv(a.sp); a.st = mv(a.st);
    a.sgeo = mv(a.sgeo); a.sirho = mv(a.sirho); a.sst = mv(a.sst);
    a.ou = mv(a.ou); a.ov = mv(a.ov); a.op = mv(a.op); a.ot = mv(a.ot); a.oq = mv(a.oq);
    a.dgeo = mv(a.dgeo); a.dirho = mv(a.dirho); a.dst = mv(a.dst);
    return a;
}

// ------------------------------------------------------------------ staged
// (blockIdx.z = ensemble member)
template <typename T>
__global__ __launch_bounds__(256) void sw2d_derive_kernel(Sw2dArgsT<T> a0) {
    const Sw2dArgsT<T> a = member_args(a0, blockIdx.z);
    __shared__ double tab[kExnerTabDoubles];
    tab[threadIdx.y * 64 + threadIdx.x] = a.exner_tab[threadIdx.y * 64 + threadIdx.x];
    __syncthreads();
    const int i = blockIdx.x * 64 + threadIdx.x;
    const int j = a.j0 + blockIdx.y * 4 + threadIdx.y;
    if (i >= a.W || j >= a.j1) return;
    const long o = (long)j * a.W + i;
    Thermo<T> th = thermo(a.sp[o], a.st[o], tab);
    a.dgeo[o] = th.geo;
    a.dirho[o] = th.t_over_p;
    a.dst[o] = th.st;
}

template <typename T, bool TEMP>
__global__ __launch_bounds__(256) void sw2d_stage_kernel(Sw2dArgsT<T> a0) {
    const Sw2dArgsT<T> a = member_args(a0, blockIdx.z);
    const int W = a.W, H = a.H;
    const int i = blockIdx.x * 64 + threadIdx.x;
    const int j = a.j0 + blockIdx.y * 4 + threadIdx.y;
    if (i >= W || j >= a.j1) return;
    const bool wrap = a.wrap_j;
    const int iw = i == 0 ? W - 1 : i - 1, ie = i == W - 1 ? 0 : i + 1;
    const long rc = row_off(j, H, W, wrap), rn = row_off(j - 1, H, W, wrap),
               rs = row_off(j + 1, H, W, wrap);
    const T uc = a.su[rc + i], uw = a.su[rc + iw], ue = a.su[rc + ie], un = a.su[rn + i], us = a.su[rs + i],
            usw = a.su[rs + iw];
    const T vc = a.sv[rc + i], vw = a.sv[rc + iw], ve = a.sv[rc + ie], vn = a.sv[rn + i], vs = a.sv[rs + i],
            vsw = a.sv[rs + iw];
    const T pc = a.sp[rc + i], pw = a.sp[rc + iw], pe = a.sp[rc + ie], pn = a.sp[rn + i], ps = a.sp[rs + i];
    T gc = pc, ge = pe, gs = ps;
    if (TEMP) {
        gc = a.sgeo[rc + i];
        ge = a.sgeo[rc + ie];
        gs = a.sgeo[rs + i];
    }
    T du = adv_vel_u(uc, uw, ue, un, us, vc, vw, vs, vsw, a.h_dx) + geo_grad(ge, gc, a.g_dx);
    T dv = adv_vel_v(vc, vw, ve, vn, vs, uc, un, uw, usw, a.h_dx) + geo_grad(gs, gc, a.g_dx);
    if (TEMP) {
        const T vis = visc_u(uc, uw, ue, un, us, a.mu_dx2) * a.sirho[rc + i];
        du -= vis;
        dv -= vis;  // the v equation uses the viscosity of u, matsumo_temp.py:75,91
    }
    const T dp = adv_geo(uc, uw, vc, vn, pc, pw, pe, pn, ps, a.h_dx);
    const long o = (long)j * W + i;
    const T bp = a.bp[o];
    const T pnew = bp - a.dt * dp;
    a.ou[o] = a.bu[o] - a.dt * du;
    a.ov[o] = a.bv[o] - a.dt * dv;
    a.op[o] = pnew;
    if (TEMP) {
        const T dst = adv_geo(uc, uw, vc, vn, a.sst[rc + i], a.sst[rc + iw], a.sst[rc + ie],
                                   a.sst[rn + i], a.sst[rs + i], a.h_dx);
        const T tt = bp * a.bt[o] - a.dt * dst;
        a.ot[o] = tt * rcp(pnew);  // unscaling, matsumo_temp.py:33-35 (dx*dx cancels)
    }
}

// one axis of the dimension-split tracer step (two_d.py:103-116), axis 0 = j with V[0] = v,
// axis 1 = i with V[1] = u
template <typename T, int AXIS, bool LIMIT>
__global__ __launch_bounds__(256) void tracer_axis_kernel(Sw2dArgsT<T> a0, const T *qin, T *qout) {
    const Sw2dArgsT<T> a = member_args(a0, blockIdx.z);
    qin += blockIdx.z * a0.mstride;
    qout += blockIdx.z * a0.mstride;
    const int W = a.W, H = a.H;
    const int i = blockIdx.x * 64 + threadIdx.x;
    const int j = a.j0 + blockIdx.y * 4 + threadIdx.y;
    if (i >= W || j >= a.j1) return;
    const bool wrap = a.wrap_j;
    T f, fm;
    const long rc = row_off(j, H, W, wrap);
    if (AXIS == 0) {
        const long r1 = row_off(j + 1, H, W, wrap), r2 = row_off(j + 2, H, W, wrap),
                   rm = row_off(j - 1, H, W, wrap), rmm = row_off(j - 2, H, W, wrap);
        const T qmm = qin[rmm + i], qm = qin[rm + i], q0 = qin[rc + i], q1 = qin[r1 + i], q2 = qin[r2 + i];
        f = face_flux<LIMIT>(a.bv[rc + i], qm, q0, q1, q2, a.dtdx);
        fm = face_flux<LIMIT>(a.bv[rm + i], qmm, qm, q0, q1, a.dtdx);
        qout[(long)j * W + i] = q0 - f + fm;
    } else {
        auto wi = [W](int x) { x %= W; return x < 0 ? x + W : x; };
        const int i1 = wi(i + 1), i2 = wi(i + 2), im = wi(i - 1), imm = wi(i - 2);
        const T qmm = qin[rc + imm], qm = qin[rc + im], q0 = qin[rc + i], q1 = qin[rc + i1], q2 = qin[rc + i2];
        f = face_flux<LIMIT>(a.bu[rc + i], qm, q0, q1, q2, a.dtdx);
        fm = face_flux<LIMIT>(a.bu[rc + im], qmm, qm, q0, q1, a.dtdx);
        qout[(long)j * W + i] = q0 - f + fm;
    }
}

template <typename T>
static dim3 cell_grid(const Sw2dArgsT<T> &a) {
    return dim3((a.W + 63) / 64, (a.j1 - a.j0 + 3) / 4, a.members);
}

template <typename T>
void launch_sw2d_derive(const Sw2dArgsT<T> &a, hipStream_t s) {
    if (a.j1 <= a.j0) return;
    hipLaunchKernelGGL(sw2d_derive_kernel<T>, cell_grid(a), dim3(64, 4), 0, s, a);
}

template <typename T>
void launch_sw2d_stage(const Sw2dArgsT<T> &a, bool temp, hipStream_t s) {
    if (a.j1 <= a.j0) return;
    if (temp)
        hipLaunchKernelGGL((sw2d_stage_kernel<T, true>), cell_grid(a), dim3(64, 4), 0, s, a);
    else
        hipLaunchKernelGGL((sw2d_stage_kernel<T, false>), cell_grid(a), dim3(64, 4), 0, s, a);
}

template <typename T>
void launch_tracer_axis(const Sw2dArgsT<T> &a, int axis, bool limit, const T *q_in, T *q_out, hipStream_t s) {
    if (a.j1 <= a.j0) return;
    dim3 g = cell_grid(a), b(64, 4);
    if (axis == 0) {
        if (limit) hipLaunchKernelGGL((tracer_axis_kernel<T, 0, true>), g, b, 0, s, a, q_in, q_out);
        else hipLaunchKernelGGL((tracer_axis_kernel<T, 0, false>), g, b, 0, s, a, q_in, q_out);
    } else {
        if (limit) hipLaunchKernelGGL((tracer_axis_kernel<T, 1, true>), g, b, 0, s, a, q_in, q_out);
        else hipLaunchKernelGGL((tracer_axis_kernel<T, 1, false>), g, b, 0, s, a, q_in, q_out);
    }
}

// ------------------------------------------------------------------ fused
// One row of a state (base or predicted) as a lane keeps it: own column and, for TEMP,
// the derived fields.
template <typename T>
struct Row {
    T u, uw, v, vw, p, st, g, irho;   // uw, vw: west neighbours, shifted once per row
};

// Where FusedCtx::iter puts an output row.  NoSink: the field arrays of the argument block, as every single-step kernel
// does.  RingSink: one row slot [field][lane] in LDS, all 64 lanes (sw2d_pair_kernel: the first step's rows, which the
// second step's wave reads back).
struct NoSink {};
template <bool TRACER>
struct RingSink {
    double *row;   // the slot, at this lane
    __device__ __forceinline__ void put(double u, double v, double p, double t, double q) const {
        row[0] = u;
        row[64] = v;
        row[128] = p;
        row[192] = t;
        if (TRACER) row[256] = q;
    }
};

template <bool TEMP, typename T>
__device__ __forceinline__ void make_row_r(Row<T> &r, T u, T v, T p, T t, const double *tab, T rcp_p) {
    r.u = u;
    r.v = v;
    r.p = p;
    r.uw = from_west(u);
    r.vw = from_west(v);
    if (TEMP) {
        Thermo<T> th = thermo(p, t, tab, rcp_p);
        r.st = th.st;
        r.g = th.geo;
        r.irho = th.t_over_p;
    } else {
        r.st = T(0.0);
        r.g = p;
        r.irho = T(0.0);
    }
}

template <bool TEMP, typename T>
__device__ __forceinline__ void make_row(Row<T> &r, T u, T v, T p, T t, const double *tab) {
    make_row_r<TEMP>(r, u, v, p, t, tab, TEMP ? rcp(p) : T(0.0));
}

template <typename T>
struct Tend {
    T du, dv, dp, dst;
};

// tendencies at the centre row R0 of a 3-row window (north RM, south RP)
template <bool TEMP, typename T>
__device__ __forceinline__ Tend<T> tendencies(const Row<T> &RM, const Row<T> &R0, const Row<T> &RP, T g_dx, T h_dx,
                                              T mu_dx2) {
    const T ue = from_east(R0.u), ve = from_east(R0.v);
    const T uw = R0.uw, vw = R0.vw, usw = RP.uw, vsw = RP.vw;
    const T pw = from_west(R0.p), pe = from_east(R0.p);
    const T ge = TEMP ? from_east(R0.g) : pe;
    Tend<T> t;
    t.du = adv_vel_u(R0.u, uw, ue, RM.u, RP.u, R0.v, vw, RP.v, vsw, h_dx) +
           geo_grad(ge, R0.g, g_dx);
    t.dv = adv_vel_v(R0.v, vw, ve, RM.v, RP.v, R0.u, RM.u, uw, usw, h_dx) +
           geo_grad(RP.g, R0.g, g_dx);
    if (TEMP) {
        const T vis = visc_u(R0.u, uw, ue, RM.u, RP.u, mu_dx2) * R0.irho;
        t.du -= vis;
        t.dv -= vis;
    }
    t.dp = adv_geo(R0.u, uw, R0.v, RM.v, R0.p, pw, pe, RM.p, RP.p, h_dx);
    t.dst = T(0.0);
    if (TEMP) {
        const T stw = from_west(R0.st), ste = from_east(R0.st);
        t.dst = adv_geo(R0.u, uw, R0.v, RM.v, R0.st, stw, ste, RM.st, RP.st, h_dx);
    }
    return t;
}

template <typename T>
struct Raw {
    T u, v, p, t, q;
};

// The deep march's stores: one output row as a buffer of W doubles, a lane's byte offset into it, and the hardware's
// range check in place of a branch around the store -- a lane that stores nothing (the halo lanes, columns >= W) passes
// kNoStore, which is beyond any row (sw2d_fused_form keeps W * 8 below it), and its store is dropped.  A branch would
// hide the stores from the compiler's count of what is in flight: it then waits for the newest requests as well.
constexpr unsigned kNoStore = 0x80000000u;
__device__ __forceinline__ void store_row_lanes(double *row, int W, unsigned lane_off, double x) {
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(row, 0, W * 8, 0x00020000);   // (raw, 32-bit)
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, x), rs, (int)lane_off, 0, 0);
}

// a copy the register coalescer cannot see through (FusedCtx::iter, the deep march); "memory": the refill of the slot
// that x came from stays behind it
__device__ __forceinline__ double own_copy(double x) {
    double y;
    asm volatile("v_mov_b64 %0, %1" : "=v"(y) : "v"(x) : "memory");
    return y;
}

// STREAM: the base state is read with nontemporal loads -- a grid far larger than the caches is read once
// per step (plus halo columns / band-edge rows), and the streaming hint is worth 1.5-2 % there (A/B on C3,
// two boxes); nontemporal STORES cost 2-8 % (a strip's 480-byte rows share their edge lines with the
// neighbouring strips, which only the L2 merges), so the results are stored normally.
// CPL: columns per lane.  2 (T = float, even W): a lane holds two neighbouring columns as one f32x2 and a wave
// marches a 120-column strip, so that its row segments stay 480 B wide as at fp64 (see launch_sw2d_fused).
template <typename T, bool TEMP, int TRACER, bool WRAPJ, bool STREAM = false, int CPL = 1>
struct FusedCtx {
    using Real = std::conditional_t<CPL == 2, f32x2, T>;   // what a lane computes on
    using V = Real;
    const Sw2dArgsT<T> &a;
    const double *tab;
    int ci, col, ja, jb;
    bool store_lane;
    V f0_prev;

    __device__ __forceinline__ Raw<V> load(int j) const {
        const long o = row_off(j, a.H, a.W, WRAPJ) + ci;
        Raw<V> r;
        if constexpr (CPL == 2) {          // ci is even and so is W: 8-byte aligned
            auto ld = [o](const T *p) {
                const f32x2 *q = (const f32x2 *)(p + o);
                return STREAM ? __builtin_nontemporal_load(q) : *q;
            };
            r.u = ld(a.bu);
            r.v = ld(a.bv);
            r.p = ld(a.bp);
            r.t = TEMP ? ld(a.bt) : V(0.0f);
            r.q = TRACER ? ld(a.bq) : V(0.0f);
        } else if (STREAM) {
            r.u = __builtin_nontemporal_load(&a.bu[o]);
            r.v = __builtin_nontemporal_load(&a.bv[o]);
            r.p = __builtin_nontemporal_load(&a.bp[o]);
            r.t = TEMP ? __builtin_nontemporal_load(&a.bt[o]) : T(0.0);
            r.q = TRACER ? __builtin_nontemporal_load(&a.bq[o]) : T(0.0);
        } else {
            r.u = a.bu[o];
            r.v = a.bv[o];
            r.p = a.bp[o];
            r.t = TEMP ? a.bt[o] : T(0.0);
            r.q = TRACER ? a.bq[o] : T(0.0);
        }
        return r;
    }

    // One row step.  On entry BM/B0/BP hold base rows r-1, r, r+1, SM/S0 the predicted rows
    // r-2, r-1; SN is a dead slot that receives predicted row r.  On exit BM's slot holds
    // base row r+2 (from the prefetched `nxt`) and `nxt` is row r+3: the caller rotates the
    // slot names instead of moving registers.
    // The deep march (sw2d_fused_kernel, DEPTH = 3) calls it with AHEAD = 5: `nxt` is then the one of three request
    // slots that holds row r+2, and it is refilled with row min(r+5, jb+1), unconditionally, so that no branch stands
    // around a load.  LEAD names what the caller knows of r: 0 r == ja-1 (neither flux nor corrector), 1 r == ja
    // (no corrector), 2 r > ja (both, unconditionally); -1: decided from r here.  ROWBUF: the deep march's stores
    // (store_row_lanes).  Sink: where the output row goes instead of the field arrays (RingSink); NoSink: the arrays.
    template <bool FETCH = true, int AHEAD = 3, int LEAD = -1, bool ROWBUF = false, class Sink = NoSink>
    __device__ __forceinline__ void iter(int r, Row<V> &BM, Row<V> &B0, Row<V> &BP, Row<V> &SN, Row<V> &SM,
                                         Row<V> &S0, Raw<V> &nxt, V &qmm, V &qm, V &q0, V &qp, Sink sink = Sink()) {
        const V dt = V(a.dt), g_dx = V(a.g_dx), h_dx = V(a.h_dx), mu_dx2 = V(a.mu_dx2), dtdx = V(a.dtdx);
        // ---- predictor: predicted row r from base rows r-1, r, r+1
        {
            const Tend<V> t = tendencies<TEMP>(BM, B0, BP, g_dx, h_dx, mu_dx2);
            const V us = B0.u - dt * t.du;
            const V vs = B0.v - dt * t.dv;
            const V ps = B0.p - dt * t.dp;
            V ts = V(0.0), rps = V(0.0);
            if (TEMP) {
                rps = rcp(ps);            // shared by the unscaling and by 1/rho of the predicted row
                ts = (B0.st - dt * t.dst) * rps;
            }
            make_row_r<TEMP>(SN, us, vs, ps, ts, tab, rps);
        }
        // ---- tracer, axis-0 flux through the face between rows r-1 and r
        V f0_cur = V(0.0);
        if (TRACER && (LEAD < 0 ? r >= ja : LEAD >= 1)) f0_cur = face_flux<TRACER == 2>(BM.v, qmm, qm, q0, qp, dtdx);
        // ---- corrector: output row r-1 from predicted rows r-2, r-1, r and base row r-1
        if (LEAD < 0 ? r >= ja + 1 : LEAD >= 2) {
            const Tend<V> t = tendencies<TEMP>(SM, S0, SN, g_dx, h_dx, mu_dx2);
            const V un = BM.u - dt * t.du;
            const V vn = BM.v - dt * t.dv;
            const V pn = BM.p - dt * t.dp;
            V tn = V(0.0), qn = V(0.0);
            if (TEMP) tn = (BM.st - dt * t.dst) * rcp(pn);
            if (TRACER) {
                const V qs = qm - f0_cur + f0_prev;  // after the axis-0 pass
                const V qs_w = from_west(qs), qs_e = from_east(qs);
                const V qs_ee = from_east(qs_e);
                const V f1 = face_flux<TRACER == 2>(BM.u, qs_w, qs, qs_e, qs_ee, dtdx);
                qn = qs - f1 + from_west(f1);
            }
            if constexpr (!std::is_same_v<Sink, NoSink>) {
                sink.put(un, vn, pn, tn, qn);
            } else if constexpr (ROWBUF) {
                const long o = (long)(r - 1) * a.W;
                const unsigned lane_off = store_lane ? (unsigned)col * 8u : kNoStore;
                store_row_lanes(a.ou + o, a.W, lane_off, un);
                store_row_lanes(a.ov + o, a.W, lane_off, vn);
                store_row_lanes(a.op + o, a.W, lane_off, pn);
                if (TEMP) store_row_lanes(a.ot + o, a.W, lane_off, tn);
                if (TRACER) store_row_lanes(a.oq + o, a.W, lane_off, qn);
            } else if (store_lane) {
                const long o = (long)(r - 1) * a.W + col;
                if constexpr (CPL == 2) {
                    auto st = [o](T *p, V x) { *(V *)(p + o) = x; };
                    st(a.ou, un);
                    st(a.ov, vn);
                    st(a.op, pn);
                    if (TEMP) st(a.ot, tn);
                    if (TRACER) st(a.oq, qn);
                } else {
                    a.ou[o] = un;
                    a.ov[o] = vn;
                    a.op[o] = pn;
                    if (TEMP) a.ot[o] = tn;
                    if (TRACER) a.oq[o] = qn;
                }
            }
        }
        // ---- slide south: the oldest base slot takes row r+2, prefetch row r+3
        f0_prev = f0_cur;
        if constexpr (AHEAD == 3) {
            make_row<TEMP>(BM, nxt.u, nxt.v, nxt.p, nxt.t, tab);
        } else {
            // The window takes copies, so that a slot's registers are dead here and the refill below lands in them
            // again.  Left to itself the compiler lets the window row and the slot trade registers from trip to trip,
            // and pays for it with moves of every slot in the loop's latch -- behind a wait for all that is in flight.
            make_row<TEMP>(BM, own_copy(nxt.u), own_copy(nxt.v), own_copy(nxt.p), TEMP ? own_copy(nxt.t) : nxt.t, tab);
        }
        if (TRACER) {
            qmm = qm;
            qm = q0;
            q0 = qp;
            if constexpr (AHEAD == 3) qp = nxt.q;
            else qp = own_copy(nxt.q);
        }
        if constexpr (AHEAD == 3) {
            if (FETCH && r + 3 <= jb + 1) nxt = load(r + 3);   // !FETCH: the caller has the rows already
        } else {
            nxt = load(min(r + AHEAD, jb + 1));
        }
    }
};

// Short bands (small grids: a band is 2-4 rows): the rows are all loaded before the first one is
// used, and the iterations are unrolled with the window slots rotated by name.  A wave then waits
// for memory once instead of once per row, which is most of its life on a 720x360 grid.
template <int N, int PRE, class Ctx, typename T = typename Ctx::Real>
__device__ __forceinline__ void preloaded_iters(Ctx &c, const Raw<T> (&pre)[PRE + 4], Row<T> &A, Row<T> &B, Row<T> &C,
                                                Row<T> &X, Row<T> &Y, Row<T> &Z, Raw<T> &nxt, T &qmm, T &qm, T &q0,
                                                T &qp) {
    if constexpr (N < PRE + 2) {
        const int r = c.ja - 1 + N;
        if (r > c.jb) return;
        c.template iter<false>(r, A, B, C, X, Y, Z, nxt, qmm, qm, q0, qp);
        if constexpr (N < PRE) nxt = pre[N + 4];          // row r + 3
        preloaded_iters<N + 1, PRE>(c, pre, B, C, A, Y, Z, X, nxt, qmm, qm, q0, qp);
    }
}

// Two columns per lane with a tracer: held to three waves per SIMD, i.e. 168 VGPRs.  Contraction within an expression
// only -- what the fp32 unit is built with, see the Makefile -- would otherwise take 170-172 VGPRs and a third of the
// waves (4096x2048 fp32 van Leer: 1.09x the time; held to 168 with 12-20 B of scratch per lane: 1.035x).  No other
// instantiation is touched: the fp64 unit's code is the same instruction for instruction.
// DEPTH: rows of requests a wave keeps in flight in the rolling march.  1: one row, asked for a row ahead of its use.
// 3 (T = double, TEMP, CPL = 1; sw2d_fused_form picks it): three request slots, one per call site of the three-row
// trip, each consumed three rows after it was asked for; that takes 162-176 VGPRs, so the kernel is held to two
// waves per SIMD (256 VGPRs) instead of the three that DEPTH = 1 reaches (profiles/deep_prefetch/).
template <typename T, bool TEMP, int TRACER, bool WRAPJ, int PRE = 0, bool STREAM = false, int CPL = 1, int DEPTH = 1>
__global__ __launch_bounds__(64, DEPTH == 3 ? 2 : (CPL == 2 && TRACER != 0) ? 3 : 1) void sw2d_fused_kernel(Sw2dArgsT<T> a0) {
    using Ctx = FusedCtx<T, TEMP, TRACER, WRAPJ, STREAM, CPL>;
    using V = typename Ctx::Real;
    constexpr int kCols = sw2d_fused_strip_cols(CPL);   // output columns per wave
    const int W = a0.W;
    const int lane = threadIdx.x;
    // Tile = (member, band, strip), strips fastest.  Workgroups are dealt round-robin over the 8
    // XCDs (b % 8 names the XCD group), each with its own L2: give every XCD a contiguous run of
    // tiles, so that neighbouring strips -- which share halo columns and the 128-B lines straddling
    // a strip edge that both write -- meet in one L2.  Speed only: any placement is correct.
    const int strips = (W + kCols - 1) / kCols;
    const int per_xcd = gridDim.x / 8;
    int tile = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
    int member = 0;
    if (a0.members > 1) {   // (one member: no integer divisions beyond the strip's -- a small grid is latency-bound)
        const int per_member = strips * ((a0.j1 - a0.j0 + a0.rows_per_band - 1) / a0.rows_per_band);
        member = tile / per_member;
        if (member >= a0.members) return;     // the padding tiles beyond the last member
        tile -= member * per_member;
    }
    const int band = tile / strips;
    const int i0 = (tile - band * strips) * kCols;
    // the member's own slab: rows wrap (row_off) inside it, no lane reads a neighbouring member
    const Sw2dArgsT<T> a = member_args(a0, member);
    __shared__ double tab[kExnerTabDoubles];
    if (TEMP) {
        for (int k = 0; k < kExnerTabDoubles / 64; ++k) tab[lane + 64 * k] = a.exner_tab[lane + 64 * k];
        __syncthreads();
    }
    Ctx c{a, tab};
    c.ja = a.j0 + band * a.rows_per_band;
    c.jb = min(c.ja + a.rows_per_band, a.j1);
    if (c.ja >= c.jb) return;   // also the padding tiles beyond the last band of a single member
    c.col = i0 - 2 * CPL + CPL * lane;   // (CPL = 2: the lane's first column; W even, so both are < W or neither)
    c.ci = c.col % W;
    if (c.ci < 0) c.ci += W;
    c.store_lane = lane >= 2 && lane < 62 && c.col < W;
    c.f0_prev = V(0.0);
    const int ja = c.ja, jb = c.jb;

    Row<V> A, B, C, X, Y, Z;
    if constexpr (PRE > 0) {               // rows_per_band <= PRE
        Raw<V> pre[PRE + 4];
#pragma unroll
        for (int n = 0; n < PRE + 4; ++n) pre[n] = c.load(min(ja - 2 + n, jb + 1));
        make_row<TEMP>(A, pre[0].u, pre[0].v, pre[0].p, pre[0].t, tab);
        make_row<TEMP>(B, pre[1].u, pre[1].v, pre[1].p, pre[1].t, tab);
        make_row<TEMP>(C, pre[2].u, pre[2].v, pre[2].p, pre[2].t, tab);
        V qmm = V(0.0), qm = pre[0].q, q0 = pre[1].q, qp = pre[2].q;
        Raw<V> nxt = pre[3];
        X = Y = Z = A;
        preloaded_iters<0, PRE>(c, pre, A, B, C, X, Y, Z, nxt, qmm, qm, q0, qp);
        return;
    }
    if constexpr (DEPTH == 3) {
        // Rows ja-2 .. ja make the window; rows ja+1 .. ja+3 fill the slots n0, n1, n2.  iter at row r consumes the
        // slot that holds row r+2 and refills it with row r+5 (clamped to jb+1, the last row a band may touch: a band
        // may be a single row).  The two rows ahead of the first output row are peeled, so that the loop's stores
        // are unconditional (store_row_lanes), and so are the last one or two rows behind the whole trips: a loop
        // with an exit behind each row is turned into one whose exits meet in the latch, where the slots in flight
        // would be moved, and so waited for, every trip.
        static_assert(PRE == 0 && CPL == 1, "the deep march is the rolling form with one column per lane");
        const Raw<V> w0 = c.load(ja - 2), w1 = c.load(ja - 1), w2 = c.load(ja);
        Raw<V> n0 = c.load(ja + 1), n1 = c.load(ja + 2), n2 = c.load(min(ja + 3, jb + 1));
        make_row<TEMP>(A, w0.u, w0.v, w0.p, w0.t, tab);
        make_row<TEMP>(B, w1.u, w1.v, w1.p, w1.t, tab);
        make_row<TEMP>(C, w2.u, w2.v, w2.p, w2.t, tab);
        V qmm = V(0.0), qm = w0.q, q0 = w1.q, qp = w2.q;
        X = Y = Z = A;  // overwritten before first use
        c.template iter<true, 5, 0, true>(ja - 1, A, B, C, X, Y, Z, n0, qmm, qm, q0, qp);
        c.template iter<true, 5, 1, true>(ja, B, C, A, Y, Z, X, n1, qmm, qm, q0, qp);
        int r = ja + 1;                   // rows ja+1 .. jb, three per trip
        for (; r + 2 <= jb; r += 3) {
            c.template iter<true, 5, 2, true>(r, C, A, B, Z, X, Y, n2, qmm, qm, q0, qp);
            c.template iter<true, 5, 2, true>(r + 1, A, B, C, X, Y, Z, n0, qmm, qm, q0, qp);
            c.template iter<true, 5, 2, true>(r + 2, B, C, A, Y, Z, X, n1, qmm, qm, q0, qp);
        }
        if (r <= jb) {                    // (the rows these would ask for are beyond jb+1)
            c.template iter<false, 3, 2, true>(r, C, A, B, Z, X, Y, n2, qmm, qm, q0, qp);
            if (r + 1 <= jb) c.template iter<false, 3, 2, true>(r + 1, A, B, C, X, Y, Z, n0, qmm, qm, q0, qp);
        }
        return;
    }
    Raw<V> x = c.load(ja - 2);
    make_row<TEMP>(A, x.u, x.v, x.p, x.t, tab);
    V qmm = V(0.0), qm = x.q;
    x = c.load(ja - 1);
    make_row<TEMP>(B, x.u, x.v, x.p, x.t, tab);
    V q0 = x.q;
    x = c.load(ja);
    make_row<TEMP>(C, x.u, x.v, x.p, x.t, tab);
    V qp = x.q;
    Raw<V> nxt = c.load(ja + 1);
    X = Y = Z = A;  // overwritten before first use

    // rows r = ja-1 .. jb, three per trip so that the window slots rotate by name
    for (int r = ja - 1; r <= jb; r += 3) {
        c.iter(r, A, B, C, X, Y, Z, nxt, qmm, qm, q0, qp);
        if (r + 1 > jb) break;
        c.iter(r + 1, B, C, A, Y, Z, X, nxt, qmm, qm, q0, qp);
        if (r + 2 > jb) break;
        c.iter(r + 2, C, A, B, Z, X, Y, nxt, qmm, qm, q0, qp);
    }
}

// ------------------------------------------------------------------ two steps per launch
// Plain shallow water on a small grid (720x360) is bound by one dependent launch per step (about
// 2.3 of 5.7 us) plus one wait for memory.  This kernel does TWO Matsuno steps per launch: a second
// pipeline of the same row-march consumes the rows of the first as they leave its corrector, three
// rows behind, and only its results go to memory.  Per step the halo grows by two cells each way:
// 56 of the 64 lanes and RPB of the RPB + 4 first-step rows are output.  Rows of the band are all
// loaded up front (compile-time indexed), the iterations are unrolled with both windows rotated by
// name.  Periodic rows only (a single band).  (kStrip2Cols: sw2d_kernels.h)

template <typename T>
struct Out3 {
    T u, v, p;
};

// predictor for row r from base rows (BM, B0, BP) into SN; corrector for row r - 1 from the
// predicted rows (SM, S0, SN) and base row BM if `corr`
template <typename T>
__device__ __forceinline__ Out3<T> matsuno_row(bool corr, const Row<T> &BM, const Row<T> &B0, const Row<T> &BP,
                                               Row<T> &SN, const Row<T> &SM, const Row<T> &S0, T dt, T g_dx, T h_dx) {
    {
        const Tend<T> t = tendencies<false>(BM, B0, BP, g_dx, h_dx, T(0.0));
        make_row<false>(SN, B0.u - dt * t.du, B0.v - dt * t.dv, B0.p - dt * t.dp, T(0.0), nullptr);
    }
    Out3<T> o{T(0.0), T(0.0), T(0.0)};
    if (corr) {
        const Tend<T> t = tendencies<false>(SM, S0, SN, g_dx, h_dx, T(0.0));
        o.u = BM.u - dt * t.du;
        o.v = BM.v - dt * t.dv;
        o.p = BM.p - dt * t.dp;
    }
    return o;
}

template <typename T>
struct Fused2Ctx {
    const Sw2dArgsT<T> &a;
    int ja, jb, col;
    bool store_lane;
};

// iteration N of RPB + 7: first-step row r1 = ja - 3 + N, second-step row r2 = r1 - 3.
// (A1..Z1) and (A2..Z2) arrive rotated: A* is the slot of the oldest base row.
template <int N, int RPB, typename T>
__device__ __forceinline__ void fused2_iters(const Fused2Ctx<T> &c, const Raw<T> (&pre)[RPB + 8], Row<T> &A1, Row<T> &B1,
                                             Row<T> &C1, Row<T> &X1, Row<T> &Y1, Row<T> &Z1, Row<T> &A2, Row<T> &B2,
                                             Row<T> &C2, Row<T> &X2, Row<T> &Y2, Row<T> &Z2) {
    if constexpr (N < RPB + 7) {
        const T dt = c.a.dt, g_dx = c.a.g_dx, h_dx = c.a.h_dx;
        const int r1 = c.ja - 3 + N;
        Out3<T> o1{T(0.0), T(0.0), T(0.0)};
        if (r1 <= c.jb + 2) {
            // first step: predicted row r1; its output row r1 - 1 once the window is primed (N >= 2)
            o1 = matsuno_row(N >= 2, A1, B1, C1, X1, Y1, Z1, dt, g_dx, h_dx);
            if constexpr (N + 3 < RPB + 8) make_row<false>(A1, pre[N + 3].u, pre[N + 3].v, pre[N + 3].p, T(0.0), nullptr);  // row r1 + 2
        }
        if constexpr (N >= 5) {
            // second step on the first step's rows: predicted row r2, output row r2 - 1 (N >= 7)
            const int r2 = r1 - 3;
            if (r2 <= c.jb) {
                const Out3<T> o2 = matsuno_row(N >= 7, A2, B2, C2, X2, Y2, Z2, dt, g_dx, h_dx);
                if (N >= 7 && r2 - 1 < c.jb && c.store_lane) {
                    const long o = (long)(r2 - 1) * c.a.W + c.col;
                    c.a.ou[o] = o2.u;
                    c.a.ov[o] = o2.v;
                    c.a.op[o] = o2.p;
                }
            }
        }
        // the first step's row r1 - 1 enters the second window: rows ja-2, ja-1, ja prime it
        // (N = 2, 3, 4), later ones replace its oldest row
        if constexpr (N >= 2) make_row<false>(A2, o1.u, o1.v, o1.p, T(0.0), nullptr);
        // rotate: pipeline 1 by one slot; pipeline 2 likewise once it runs or is being primed
        if constexpr (N >= 2)
            fused2_iters<N + 1, RPB>(c, pre, B1, C1, A1, Y1, Z1, X1, B2, C2, A2, Y2, Z2, X2);
        else
            fused2_iters<N + 1, RPB>(c, pre, B1, C1, A1, Y1, Z1, X1, A2, B2, C2, X2, Y2, Z2);
    }
}

// ENS: an ensemble launch.  One member compiles to the code without a member: this kernel is bound by the
// latency of its first loads, and the member's bookkeeping in front of them cost 1-2 % at C2.
template <typename T, int RPB, bool ENS>
__global__ __launch_bounds__(64) void sw2d_fused2_kernel(Sw2dArgsT<T> a0) {
    const int W = a0.W, H = a0.H;
    const int lane = threadIdx.x;
    // tiles (member, band, strip) as in sw2d_fused_kernel
    const int strips = (W + kStrip2Cols - 1) / kStrip2Cols;
    const int per_xcd = gridDim.x / 8;
    int tile = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
    int member = 0;
    if constexpr (ENS) {
        const int per_member = strips * ((H + RPB - 1) / RPB);
        member = tile / per_member;
        if (member >= a0.members) return;
        tile -= member * per_member;
    }
    const int band = tile / strips;
    const int i0 = (tile - band * strips) * kStrip2Cols;
    const Sw2dArgsT<T> a = ENS ? member_args(a0, member) : a0;
    Fused2Ctx<T> c{a};
    c.ja = a.j0 + band * RPB;
    c.jb = min(c.ja + RPB, a.j1);
    if (c.ja >= c.jb) return;
    c.col = i0 - 4 + lane;
    int ci = c.col % W;
    if (ci < 0) ci += W;
    c.store_lane = lane >= 4 && lane < 60 && c.col < W;
    Raw<T> pre[RPB + 8];                         // rows ja - 4 .. ja + RPB + 3, periodic in j
#pragma unroll
    for (int n = 0; n < RPB + 8; ++n) {
        int j = (c.ja - 4 + n) % H;
        if (j < 0) j += H;
        const long o = (long)j * W + ci;
        pre[n].u = a.bu[o];
        pre[n].v = a.bv[o];
        pre[n].p = a.bp[o];
        pre[n].t = T(0.0);
        pre[n].q = T(0.0);
    }
    Row<T> A1, B1, C1, X1, Y1, Z1, A2, B2, C2, X2, Y2, Z2;
    make_row<false>(A1, pre[0].u, pre[0].v, pre[0].p, T(0.0), nullptr);
    make_row<false>(B1, pre[1].u, pre[1].v, pre[1].p, T(0.0), nullptr);
    make_row<false>(C1, pre[2].u, pre[2].v, pre[2].p, T(0.0), nullptr);
    X1 = Y1 = Z1 = A2 = B2 = C2 = X2 = Y2 = Z2 = A1;       // overwritten before first use
    fused2_iters<0, RPB>(c, pre, A1, B1, C1, X1, Y1, Z1, A2, B2, C2, X2, Y2, Z2);
}

// two Matsuno steps of GCM_SW2D in one launch; needs wrap_j, rows_per_band in 2..4
template <typename T>
bool launch_sw2d_fused2(const Sw2dArgsT<T> &a, hipStream_t s) {
    if (!sw2d_fused2_serves(a.wrap_j, a.j0, a.j1, a.H, a.rows_per_band)) return false;
    const int strips = (a.W + kStrip2Cols - 1) / kStrip2Cols;
    const int bands = (a.H + a.rows_per_band - 1) / a.rows_per_band;
    dim3 g((unsigned)(((long)strips * bands * a.members + 7) / 8 * 8));
    Sw2dArgsT<T> arg = a;
    void *params[] = {&arg};
    const bool ens = a.members > 1;
    const void *fn = a.rows_per_band == 2 ? (ens ? (const void *)sw2d_fused2_kernel<T, 2, true> : (const void *)sw2d_fused2_kernel<T, 2, false>)
                   : a.rows_per_band == 3 ? (ens ? (const void *)sw2d_fused2_kernel<T, 3, true> : (const void *)sw2d_fused2_kernel<T, 3, false>)
                                          : (ens ? (const void *)sw2d_fused2_kernel<T, 4, true> : (const void *)sw2d_fused2_kernel<T, 4, false>);
    return hipLaunchKernel(fn, g, dim3(64), params, 0, s) == hipSuccess;
}

// ------------------------------------------------------------------ two steps per launch, streaming grids
// GCM_SW2D_TEMP at float64 on a grid far beyond the caches: the deep march is on the memory ceiling of its access
// pattern, and every step sends the whole state to HBM and fetches it back.  Here a workgroup of TWO waves owns a tile
// (band, 56-column strip) and does two Matsuno steps: wave 0 is the deep march (three request slots, clamped refill,
// peeled rows, own_copy) over the band extended by two rows each way, [ja - 2, jb + 2), and its output rows go to a
// ring of row slots in LDS; wave 1 runs the second step on those rows -- FusedCtx::iter in the form that takes rows
// the caller already has -- and stores rows [ja, jb).  Lane <-> column is the same in both waves, col = i0 - 4 + lane;
// the first step is valid on lanes 2 .. 61, the second on lanes 4 .. 59, so a ring row is [field][lane].  A second
// pipeline inside ONE wave (sw2d_fused2_kernel) needs about 250-260 VGPRs with theta and a tracer; here each wave keeps
// the footprint of the single-step march.
//
// Trips and barriers.  A trip is three rows.  The first step's output rows are numbered k = 0 .. rows + 3 (row
// ja - 2 + k); wave 0 writes rows 3t .. 3t + 2 in trip t, into ring rows k % 6, i.e. the ring is two groups of three
// rows and trip t writes group t & 1.  Wave 1 reads, in trip t >= 1, the group trip t - 1 wrote: rows 0 .. 2 make its
// window in trip 1, and from trip 2 on row k = n + 3 is the row r + 2 that its n-th iter (r = ja - 1 + n) slides in.
// ONE __syncthreads() ends every trip of either wave, nothing else synchronises them: the group a wave touches in trip
// t is the one the other wave touched in trip t - 1 and will touch in trip t + 1.  Both waves take 3 + (rows + 1) / 3
// trips -- wave 1 has the rows + 2 iters of a band behind two trips of waiting; wave 0 needs ceil((rows + 4) / 3) and
// takes the barriers of the trips it has nothing to do in -- which depends on the band's row count alone, and no barrier
// stands under a lane mask: the role is wave-uniform.  The last rows wave 1 slides in (beyond k = rows + 3) are whatever
// the ring holds; they enter window rows no output row reads.
constexpr int kPairRowDoubles = 5 * 64;                 // a ring row: [field][lane]
constexpr int kPairGroupDoubles = 3 * kPairRowDoubles;  // the ring: two groups of three rows (15 KB)

template <int TRACER, bool STREAM>
__global__ __launch_bounds__(128, 2) void sw2d_pair_kernel(Sw2dArgsT<double> a) {
    using Ctx = FusedCtx<double, true, TRACER, true, STREAM, 1>;
    using Sink = RingSink<TRACER != 0>;
    const int W = a.W;
    const int lane = threadIdx.x & 63;
    const int role = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // tiles (band, strip) as in sw2d_fused_kernel, one member
    const int strips = (W + kStrip2Cols - 1) / kStrip2Cols;
    const int per_xcd = gridDim.x / 8;
    const int tile = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
    const int band = tile / strips;
    const int i0 = (tile - band * strips) * kStrip2Cols;
    __shared__ double tab[kExnerTabDoubles];
    __shared__ double ring[2 * kPairGroupDoubles];
    for (int k = 0; k < kExnerTabDoubles / 128; ++k) tab[threadIdx.x + 128 * k] = a.exner_tab[threadIdx.x + 128 * k];
    __syncthreads();
    const int ja = band * a.rows_per_band;          // (all rows of a periodic grid: sw2d_pair_serves)
    const int jb = min(ja + a.rows_per_band, a.H);
    if (ja >= jb) return;                           // the padding tiles: both waves leave
    const int col = i0 - 4 + lane;
    Ctx c{a, tab};
    c.col = col;
    c.ci = col % W;
    if (c.ci < 0) c.ci += W;
    c.f0_prev = 0.0;
    Row<double> A, B, C, X, Y, Z;
    int g = 0;                                      // the group of this trip, as an offset into the ring
    if (role == 0) {
        // ---- the first step: the deep march of sw2d_fused_kernel over [ja - 2, jb + 2), rows to the ring
        c.ja = ja - 2;
        c.jb = jb + 2;
        c.store_lane = false;
        const int j0 = c.ja, j1 = c.jb;
        int left = 3 + (jb - ja + 1) / 3;           // barriers still to take
        double *const slot = ring + lane;
        const Raw<double> w0 = c.load(j0 - 2), w1 = c.load(j0 - 1), w2 = c.load(j0);
        Raw<double> n0 = c.load(j0 + 1), n1 = c.load(j0 + 2), n2 = c.load(j0 + 3);   // (j0 + 3 < j1 + 1)
        make_row<true>(A, w0.u, w0.v, w0.p, w0.t, tab);
        make_row<true>(B, w1.u, w1.v, w1.p, w1.t, tab);
        make_row<true>(C, w2.u, w2.v, w2.p, w2.t, tab);
        double qmm = 0.0, qm = w0.q, q0 = w1.q, qp = w2.q;
        X = Y = Z = A;  // overwritten before first use
        c.template iter<true, 5, 0, true>(j0 - 1, A, B, C, X, Y, Z, n0, qmm, qm, q0, qp);
        c.template iter<true, 5, 1, true>(j0, B, C, A, Y, Z, X, n1, qmm, qm, q0, qp);
        int r = j0 + 1;                   // rows j0+1 .. j1, three per trip
        for (; r + 2 <= j1; r += 3) {
            c.template iter<true, 5, 2, true>(r, C, A, B, Z, X, Y, n2, qmm, qm, q0, qp, Sink{slot + g});
            c.template iter<true, 5, 2, true>(r + 1, A, B, C, X, Y, Z, n0, qmm, qm, q0, qp, Sink{slot + g + kPairRowDoubles});
            c.template iter<true, 5, 2, true>(r + 2, B, C, A, Y, Z, X, n1, qmm, qm, q0, qp, Sink{slot + g + 2 * kPairRowDoubles});
            g ^= kPairGroupDoubles;
            __syncthreads();
            --left;
        }
        if (r <= j1) {                    // (the rows these would ask for are beyond j1+1)
            c.template iter<false, 3, 2, true>(r, C, A, B, Z, X, Y, n2, qmm, qm, q0, qp, Sink{slot + g});
            if (r + 1 <= j1) c.template iter<false, 3, 2, true>(r + 1, A, B, C, X, Y, Z, n0, qmm, qm, q0, qp, Sink{slot + g + kPairRowDoubles});
            __syncthreads();
            --left;
        }
        for (; left > 0; --left) __syncthreads();   // the trips in which only the second step has rows
    } else {
        // ---- the second step on the ring's rows: rows [ja, jb) to memory
        c.ja = ja;
        c.jb = jb;
        c.store_lane = lane >= 4 && lane < 60 && col < W;
        const double *const slot = ring + lane;
        auto rd = [slot](int off) {
            const double *p = slot + off;
            Raw<double> x;
            x.u = p[0];
            x.v = p[64];
            x.p = p[128];
            x.t = p[192];
            x.q = TRACER ? p[256] : 0.0;
            return x;
        };
        __syncthreads();                  // trip 0: nothing to read yet
        const Raw<double> w0 = rd(0), w1 = rd(kPairRowDoubles), w2 = rd(2 * kPairRowDoubles);   // rows ja-2 .. ja
        make_row<true>(A, w0.u, w0.v, w0.p, w0.t, tab);
        make_row<true>(B, w1.u, w1.v, w1.p, w1.t, tab);
        make_row<true>(C, w2.u, w2.v, w2.p, w2.t, tab);
        double qmm = 0.0, qm = w0.q, q0 = w1.q, qp = w2.q;
        X = Y = Z = A;  // overwritten before first use
        __syncthreads();                  // trip 1: the window
        g = kPairGroupDoubles;
        // trip 2: the two rows ahead of the first output row and that row, as the deep march peels them (a band has
        // rows + 2 >= 3 iters)
        Raw<double> nxt = rd(g);
        c.template iter<false, 3, 0, true>(ja - 1, A, B, C, X, Y, Z, nxt, qmm, qm, q0, qp);
        nxt = rd(g + kPairRowDoubles);
        c.template iter<false, 3, 1, true>(ja, B, C, A, Y, Z, X, nxt, qmm, qm, q0, qp);
        nxt = rd(g + 2 * kPairRowDoubles);
        c.template iter<false, 3, 2, true>(ja + 1, C, A, B, Z, X, Y, nxt, qmm, qm, q0, qp);
        g ^= kPairGroupDoubles;
        __syncthreads();
        int r = ja + 2;                   // rows ja+2 .. jb, three per trip
        for (; r + 2 <= jb; r += 3) {
            nxt = rd(g);
            c.template iter<false, 3, 2, true>(r, A, B, C, X, Y, Z, nxt, qmm, qm, q0, qp);
            nxt = rd(g + kPairRowDoubles);
            c.template iter<false, 3, 2, true>(r + 1, B, C, A, Y, Z, X, nxt, qmm, qm, q0, qp);
            nxt = rd(g + 2 * kPairRowDoubles);
            c.template iter<false, 3, 2, true>(r + 2, C, A, B, Z, X, Y, nxt, qmm, qm, q0, qp);
            g ^= kPairGroupDoubles;
            __syncthreads();
        }
        if (r <= jb) {
            nxt = rd(g);
            c.template iter<false, 3, 2, true>(r, A, B, C, X, Y, Z, nxt, qmm, qm, q0, qp);
            if (r + 1 <= jb) {
                nxt = rd(g + kPairRowDoubles);
                c.template iter<false, 3, 2, true>(r + 1, B, C, A, Y, Z, X, nxt, qmm, qm, q0, qp);
            }
            __syncthreads();
        }
    }
}

template <typename T>
static const void *pair_kernel_ptr(int tracer, bool stream) {
    static_assert(std::is_same_v<T, double>, "the wave pair exists at float64 only");
    if (tracer == 0) return stream ? (const void *)sw2d_pair_kernel<0, true> : (const void *)sw2d_pair_kernel<0, false>;
    if (tracer == 1) return stream ? (const void *)sw2d_pair_kernel<1, true> : (const void *)sw2d_pair_kernel<1, false>;
    return stream ? (const void *)sw2d_pair_kernel<2, true> : (const void *)sw2d_pair_kernel<2, false>;
}

// Rows per workgroup of the wave pair: one resident round -- as many workgroups as the chip holds at the kernel's
// footprint (C3: 4 per CU, 1024; 74 strips x 13 bands of 158 rows).  GCM_SW2D_PAIR_ROWS pins it.
template <typename T>
int sw2d_pair_rows_per_band(int W, int H, int tracer, bool stream) {
    if (const char *e = getenv("GCM_SW2D_PAIR_ROWS")) {
        int v = atoi(e);
        if (v > 0) return v;
    }
    int wgs_per_cu = 4, cus = 256, dev = 0, nb = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
        cus = prop.multiProcessorCount;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, pair_kernel_ptr<T>(tracer, stream), 128, 0) == hipSuccess && nb > 0)
        wgs_per_cu = nb;
    const long strips = (W + kStrip2Cols - 1) / kStrip2Cols;
    long bands = (long)wgs_per_cu * cus / strips;   // floor: stay within the round
    if (bands < 1) bands = 1;
    const long rpb = (H + bands - 1) / bands;
    return (int)(rpb < 8 ? 8 : rpb);
}

// two Matsuno steps of float64 GCM_SW2D_TEMP in one launch (sw2d_pair_serves); false: refused
template <typename T>
bool launch_sw2d_pair(const Sw2dArgsT<T> &a, int tracer, bool stream, hipStream_t s) {
    if (!sw2d_pair_serves(a.wrap_j, a.j0, a.j1, a.H, a.W, a.members, a.rows_per_band)) return false;
    const int strips = (a.W + kStrip2Cols - 1) / kStrip2Cols;
    const int bands = (a.H + a.rows_per_band - 1) / a.rows_per_band;
    dim3 g((unsigned)(((long)strips * bands + 7) / 8 * 8));
    Sw2dArgsT<T> arg = a;
    void *params[] = {&arg};
    return hipLaunchKernel(pair_kernel_ptr<T>(tracer, stream), g, dim3(128), params, 0, s) == hipSuccess;
}

template <typename T, bool TEMP, int TRACER, int CPL = 1>
static const void *fused_fn(bool wrap, bool stream, int depth = 1) {
    if constexpr (std::is_same_v<T, double> && TEMP && CPL == 1) {   // the deep march exists for these only
        if (depth == 3) {
            if (stream)
                return wrap ? (const void *)sw2d_fused_kernel<T, TEMP, TRACER, true, 0, true, CPL, 3>
                            : (const void *)sw2d_fused_kernel<T, TEMP, TRACER, false, 0, true, CPL, 3>;
            return wrap ? (const void *)sw2d_fused_kernel<T, TEMP, TRACER, true, 0, false, CPL, 3>
                        : (const void *)sw2d_fused_kernel<T, TEMP, TRACER, false, 0, false, CPL, 3>;
        }
    }
    if (stream)
        return wrap ? (const void *)sw2d_fused_kernel<T, TEMP, TRACER, true, 0, true, CPL>
                    : (const void *)sw2d_fused_kernel<T, TEMP, TRACER, false, 0, true, CPL>;
    return wrap ? (const void *)sw2d_fused_kernel<T, TEMP, TRACER, true, 0, false, CPL>
                : (const void *)sw2d_fused_kernel<T, TEMP, TRACER, false, 0, false, CPL>;
}

// (preload, stream: sw2d_fused_form; kPreloadRows: sw2d_kernels.h)
template <typename T, int CPL>
static const void *fused_kernel_ptr_c(bool temp, int tracer, bool wrap, bool preload, bool stream, int depth) {
    if (!temp) {
        if (preload)
            return wrap ? (const void *)sw2d_fused_kernel<T, false, 0, true, kPreloadRows, false, CPL>
                        : (const void *)sw2d_fused_kernel<T, false, 0, false, kPreloadRows, false, CPL>;
        return fused_fn<T, false, 0, CPL>(wrap, stream);
    }
    if (tracer == 0) return fused_fn<T, true, 0, CPL>(wrap, stream, depth);
    if (tracer == 1) return fused_fn<T, true, 1, CPL>(wrap, stream, depth);
    return fused_fn<T, true, 2, CPL>(wrap, stream, depth);
}

// stream: the rows this launch reads are far more than the caches hold (see FusedCtx); cols: columns per lane
// (2: T = float and an even width only); depth: rows of requests in flight (3: T = double with temp only)
template <typename T>
static const void *fused_kernel_ptr(bool temp, int tracer, bool wrap, bool preload = false, bool stream = false,
                                    int cols = 1, int depth = 1) {
    if constexpr (std::is_same_v<T, float>)
        if (cols == 2) return fused_kernel_ptr_c<T, 2>(temp, tracer, wrap, preload, stream, 1);
    return fused_kernel_ptr_c<T, 1>(temp, tracer, wrap, preload, stream, depth);
}

// Rows per wave.  Large grids: one resident round -- as many waves as the chip holds at
// this kernel's register footprint (a second, partly filled round would idle most SIMDs
// at the tail); small grids: short bands so that every SIMD gets a wave.  An ensemble counts
// the waves of all `members` grids: short bands exist only to fill the chip, and once M
// members fill it the 4 halo rows of a short band are pure overhead.
// The deep march (sw2d_fused_form: depth 3) holds fewer waves, and its occupancy is asked of the kernel that runs; it
// takes as many resident rounds as keep a band within kDeepMaxRows rows (C3: one round, 69 strips x 29 bands of 71).
constexpr int kDeepMaxRows = 96;
template <typename T>
int sw2d_fused_rows_per_band(int W, int H, bool temp, int tracer, bool wrap, int members, int cols, int depth_pin) {
    if (const char *e = getenv("GCM_FUSED_ROWS")) {
        int v = atoi(e);
        if (v > 0) return v;
    }
    const long M = members < 1 ? 1 : members;
    // (the band length is not known yet: it matters to the form of plain shallow water only, which has no deep march)
    const Sw2dFusedForm form = sw2d_fused_form(temp, tracer, kPreloadRows + 1, W, H, M, (long)sizeof(T), depth_pin);
    const bool deep = form.depth == 3;
    int waves_per_cu = deep ? 8 : 12, cus = 256, dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
        cus = prop.multiProcessorCount;
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fused_kernel_ptr<T>(temp, tracer, wrap, false, deep && form.stream, cols, form.depth),
                                                     64, 0) == hipSuccess && nb > 0)
        waves_per_cu = nb;
    const long slots = (long)waves_per_cu * cus;
    const long strips = (W + sw2d_fused_strip_cols(cols) - 1) / sw2d_fused_strip_cols(cols);
    auto waves = [&](int rpb) { return M * strips * ((H + rpb - 1) / rpb); };
    if (deep && waves(8) >= slots) {
        for (long rounds = 1;; ++rounds) {
            long bands = rounds * slots / (strips * M);   // per member; floor: stay within `rounds` full rounds
            if (bands < 1) bands = 1;
            const long rpb = (H + bands - 1) / bands;
            if (rpb <= kDeepMaxRows || bands >= H) return (int)(rpb < 8 ? 8 : rpb);
        }
    }
    if (waves(8) < slots) {  // small grid: aim at one wave per SIMD at least
        long rpb = M * H * strips / (5L * cus);   // ~1.3 waves per SIMD (measured best on 720x360)
        // plain SW2D ensembles that do not fill the chip at 8 rows: bands short enough for two steps per launch
        // (sw2d_fused2_kernel), which halves the launches and the state's round trips -- 0.85x the time of 8-row
        // bands at 360x180, M = 16 (tools/tools_ensemble_time.py --only rows)
        if (!temp && M > 1 && rpb > kPreloadRows) rpb = kPreloadRows;
        return (int)(rpb < 2 ? 2 : rpb > 8 ? 8 : rpb);
    }
    long rounds = (waves(64) + slots - 1) / slots;
    long bands = rounds * slots / (strips * M);  // per member; floor: stay within `rounds` full rounds
    if (bands < 1) bands = 1;
    long rpb = (H + bands - 1) / bands;
    return (int)(rpb < 8 ? 8 : rpb);
}

// Columns per lane of the fused kernel.  Two (float, even width) halve the waves and keep a wave's row segments
// at 480 B: C3 0.86x and the 32 x 720x360 ensemble 0.84x the time of one column per lane, but a grid too small
// to fill the chip at 8-row bands is bound by latency, and there half the waves cost (C2 1.06x; A/B in
// profiles/sw2d_f32/f32_cols_ab.jsonl).  So: two columns once the one-column kernel fills the chip.
template <typename T>
int sw2d_fused_cols(int W, int H, bool temp, int tracer, bool wrap, int members) {
    if (!std::is_same_v<T, float> || W % 2) return 1;
    if (const char *e = getenv("GCM_SW2D_F32_COLS")) return e[0] == '1' ? 1 : 2;
    int waves_per_cu = 12, cus = 256, dev = 0, nb = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
        cus = prop.multiProcessorCount;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fused_kernel_ptr<T>(temp, tracer, wrap), 64, 0) == hipSuccess &&
        nb > 0)
        waves_per_cu = nb;
    const long strips = (W + kStripCols - 1) / kStripCols;
    const long waves8 = (long)(members < 1 ? 1 : members) * strips * ((H + 7) / 8);
    return waves8 < (long)waves_per_cu * cus ? 1 : 2;
}

template <typename T>
bool launch_sw2d_fused(const Sw2dArgsT<T> &a, bool temp, int tracer, hipStream_t s, int cols, int depth_pin) {
    if (a.j1 <= a.j0) return true;
    const int strips = (a.W + sw2d_fused_strip_cols(cols) - 1) / sw2d_fused_strip_cols(cols);
    const int bands = (a.j1 - a.j0 + a.rows_per_band - 1) / a.rows_per_band;
    dim3 g((unsigned)(((long)strips * bands * a.members + 7) / 8 * 8));  // 1-D, padded to 8 XCD groups
    Sw2dArgsT<T> arg = a;
    void *params[] = {&arg};
    // fields x sizeof(T) bytes x the rows of this launch (all members), read once: stream it when that is beyond the
    // 256 MB Infinity Cache (sw2d_fused_form)
    const Sw2dFusedForm f = sw2d_fused_form(temp, tracer, a.rows_per_band, a.W, a.j1 - a.j0, a.members, (long)sizeof(T), depth_pin);
    return hipLaunchKernel(fused_kernel_ptr<T>(temp, tracer, a.wrap_j != 0, f.preload, f.stream, cols, f.depth), g, dim3(64), params, 0, s) == hipSuccess;
}

template <typename T>
__global__ void copy_rows_kernel(T *dst, const T *src, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; i < n; i += stride) dst[i] = src[i];
}

template <typename T>
void launch_copy_rows(T *dst, const T *src, int W, int nrows, hipStream_t s) {
    const long n = (long)W * nrows;
    if (n <= 0) return;
    int blocks = (int)((n + 255) / 256);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(copy_rows_kernel<T>, dim3(blocks), dim3(256), 0, s, dst, src, n);
}

// the launchers of one real type (sw2d_kernels.h)
#define GCM_SW2D_INSTANTIATE(T)                                                                                   \
    template void launch_sw2d_stage<T>(const Sw2dArgsT<T> &, bool, hipStream_t);                                 \
    template void launch_sw2d_derive<T>(const Sw2dArgsT<T> &, hipStream_t);                                      \
    template void launch_tracer_axis<T>(const Sw2dArgsT<T> &, int, bool, const T *, T *, hipStream_t);           \
    template bool launch_sw2d_fused<T>(const Sw2dArgsT<T> &, bool, int, hipStream_t, int, int);                  \
    template int sw2d_fused_rows_per_band<T>(int, int, bool, int, bool, int, int, int);                         \
    template int sw2d_fused_cols<T>(int, int, bool, int, bool, int);                                            \
    template bool launch_sw2d_fused2<T>(const Sw2dArgsT<T> &, hipStream_t);                                      \
    template void launch_copy_rows<T>(T *, const T *, int, int, hipStream_t);

}  // namespace gcm

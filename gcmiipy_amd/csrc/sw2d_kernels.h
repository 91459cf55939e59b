// Kernel argument block + launch prototypes for the 2-D shallow-water family
// (GCM_SW2D, GCM_SW2D_TEMP [+ tracer]).
#pragma once
#include <hip/hip_runtime.h>

namespace gcm {

constexpr int kExnerTabDoubles = 256;  // [0,128): E_e, e = -64..63; then 64 x {rc_i, ck_i}
constexpr int kGhost = 2;        // ghost rows on each side of a latitude band
constexpr int kStripCols = 60;   // output columns per wave in the fused kernel (64 lanes - 2x2 halo)

constexpr int kStrip2Cols = 56;  // output columns per wave in the two-step kernel (64 lanes - 2x4: the halo of two steps)
constexpr int kPreloadRows = 4;  // bands of up to this many rows use the preloading variant (plain SW2D)

// The launch geometry of the fused kernels: the expressions the launchers (sw2d_impl.h) and the read-only query
// gcm_sw2d_plan (gcmcore.hip) share, so that the query cannot drift from the launch.
// output columns per wave of the single-step kernel with `cols` columns per lane
constexpr int sw2d_fused_strip_cols(int cols) { return cols * kStripCols; }
// whether the two-step kernel serves a launch: periodic rows, all of them, bands of 2..4 rows
inline bool sw2d_fused2_serves(int wrap_j, int j0, int j1, int H, int rows_per_band) {
    return wrap_j && j0 == 0 && j1 == H && rows_per_band >= 2 && rows_per_band <= 4;
}
// whether the wave pair (sw2d_pair_kernel: two steps of float64 GCM_SW2D_TEMP per launch) serves a launch: periodic
// rows, all of them, one member, a width whose rows the second step's buffer stores address (as the deep march's)
inline bool sw2d_pair_serves(int wrap_j, int j0, int j1, int H, long W, int members, int rows_per_band) {
    return wrap_j && j0 == 0 && j1 == H && members == 1 && rows_per_band >= 1 && W < (1L << 27);
}
// the form of the single-step kernel: preloading (plain SW2D, short bands) or rolling, and the rolling one's STREAM
// instantiation where the rows of one launch (all members, `esz` bytes an element) are beyond the 256 MB Infinity Cache
// depth: rows of requests a wave of the rolling form keeps in flight.  3 -- the deep march, two waves per SIMD -- where
// the launch streams, the model is GCM_SW2D_TEMP, the state is float64 and the handle has one member: a grid that size
// leaves HBM waiting on the one row a wave has asked for.  A property of the grid, the same on every call.  `pin` (GCM_SW2D_DEPTH = 1 | 3, kept
// in the handle; 0: none) fixes the depth of a float64 GCM_SW2D_TEMP launch of any size; nothing else has a deep form.
struct Sw2dFusedForm {
    bool preload, stream;
    int depth;
};
inline Sw2dFusedForm sw2d_fused_form(bool temp, int tracer, int rows_per_band, long W, long rows, long members,
                                     long esz, int pin = 0) {
    const int nfields = 3 + (temp ? 1 : 0) + (tracer ? 1 : 0);
    const bool preload = !temp && rows_per_band <= kPreloadRows;
    const bool stream = !preload && W * rows * members * esz * nfields > (256L << 20);
    // (W: the deep march stores through one buffer per row, whose size in bytes and whose no-store offset are 32-bit)
    // (one member: an ensemble's members stay bit for bit what single handles of their size compute, which is depth 1)
    const bool deep = temp && esz == 8 && !preload && W < (1L << 27) && (pin ? pin == 3 : stream && members == 1);
    return {preload, stream, deep ? 3 : 1};
}

// Pointers address interior row 0 of member 0; with wrap_j == 0 rows -2,-1 and H,H+1 are ghost rows.
// Member m's field starts mstride elements after member m-1's (an ensemble handle, members > 1).
// T is the real type of the state and of the arithmetic: double, or float for an fp32 handle.
template <typename T>
struct Sw2dArgsT {
    const T *bu, *bv, *bp, *bt, *bq;        // base (time n) state
    const T *su, *sv, *sp, *st;             // stage state the tendencies are evaluated on
    const T *sgeo, *sirho, *sst;            // staged TEMP: geo, T/p, p*t of the stage state
    T *ou, *ov, *op, *ot, *oq;              // output
    T *dgeo, *dirho, *dst;                  // derive kernel outputs
    const double *exner_tab;                // device copy of the 256-double exner table (float64 for either T)
    int W, H;                               // columns, rows owned
    int wrap_j;                             // 1: rows wrap modulo H (single band); 0: ghost rows
    int j0, j1;                             // row range [j0, j1) to produce
    int rows_per_band;                      // fused: output rows per wave
    int members;                            // ensemble members M (>= 1): one launch advances all of them
    long mstride;                           // elements from one member's slab to the next (every pointer above)
    T dt, dx, inv_dx, dx2, inv_dx2;
    T h_dx;                                 // 0.5 / dx (exact halving folded in)
    T dtdx;                                 // dt / dx
    T g_dx, mu_dx2, inv_dx2_;               // G / dx, mu_air Rd / dx^2, 1 / dx^2
};
using Sw2dArgs = Sw2dArgsT<double>;

// an fp32 handle's argument block: the same addresses, the scalars (formed in float64) rounded once
inline Sw2dArgsT<float> narrow_args(const Sw2dArgs &a) {
    Sw2dArgsT<float> f{};
    auto cp = [](auto *p) { return (float *)p; };
    f.bu = cp(a.bu); f.bv = cp(a.bv); f.bp = cp(a.bp); f.bt = cp(a.bt); f.bq = cp(a.bq);
    f.su = cp(a.su); f.sv = cp(a.sv); f.sp = cp(a.sp); f.st = cp(a.st);
    f.sgeo = cp(a.sgeo); f.sirho = cp(a.sirho); f.sst = cp(a.sst);
    f.ou = cp(a.ou); f.ov = cp(a.ov); f.op = cp(a.op); f.ot = cp(a.ot); f.oq = cp(a.oq);
    f.dgeo = cp(a.dgeo); f.dirho = cp(a.dirho); f.dst = cp(a.dst);
    f.exner_tab = a.exner_tab;
    f.W = a.W; f.H = a.H; f.wrap_j = a.wrap_j; f.j0 = a.j0; f.j1 = a.j1;
    f.rows_per_band = a.rows_per_band; f.members = a.members; f.mstride = a.mstride;
    f.dt = (float)a.dt; f.dx = (float)a.dx; f.inv_dx = (float)a.inv_dx; f.dx2 = (float)a.dx2;
    f.inv_dx2 = (float)a.inv_dx2; f.h_dx = (float)a.h_dx; f.dtdx = (float)a.dtdx; f.g_dx = (float)a.g_dx;
    f.mu_dx2 = (float)a.mu_dx2; f.inv_dx2_ = (float)a.inv_dx2_;
    return f;
}

// Launchers, instantiated for T = double (sw2d_kernels.hip) and T = float (sw2d_kernels_f32.hip).
// staged variant
template <typename T> void launch_sw2d_stage(const Sw2dArgsT<T> &a, bool temp, hipStream_t s);
template <typename T> void launch_sw2d_derive(const Sw2dArgsT<T> &a, hipStream_t s);   // p,t -> geo, 1/rho, scaled_t
template <typename T>
void launch_tracer_axis(const Sw2dArgsT<T> &a, int axis, bool limit, const T *q_in, T *q_out, hipStream_t s);
// fused variant: predictor + corrector (+ both tracer passes) in one launch
// cols: columns per lane, 1 (60-column strips) or 2 (T = float with an even width: 120-column strips of 8-byte
// requests, so that a row segment is 480 B as at fp64)
// depth_pin: the handle's GCM_SW2D_DEPTH (sw2d_fused_form), 0 for none
template <typename T>
bool launch_sw2d_fused(const Sw2dArgsT<T> &a, bool temp, int tracer, hipStream_t s, int cols = 1,
                       int depth_pin = 0);   // false: refused
template <typename T>
int sw2d_fused_rows_per_band(int W, int H, bool temp, int tracer, bool wrap, int members = 1, int cols = 1,
                             int depth_pin = 0);
// the columns per lane a handle's fused launches use: 1 for double and odd widths; float: 2 once the grid (all
// members) fills the chip, GCM_SW2D_F32_COLS=1 / 2 overrides
template <typename T> int sw2d_fused_cols(int W, int H, bool temp, int tracer, bool wrap, int members);
// GCM_SW2D, single band, short bands (small grids): TWO steps in one launch; false if not applicable
template <typename T> bool launch_sw2d_fused2(const Sw2dArgsT<T> &a, hipStream_t s);
// float64 GCM_SW2D_TEMP, periodic single domain, one member: TWO steps in one launch by a pair of waves per tile, the
// first step's rows handed over in LDS (T = double only); a.rows_per_band is the pair's own band length, which
// sw2d_pair_rows_per_band chooses: one resident round of workgroups, or GCM_SW2D_PAIR_ROWS.  false: refused
template <typename T> bool launch_sw2d_pair(const Sw2dArgsT<T> &a, int tracer, bool stream, hipStream_t s);
template <typename T> int sw2d_pair_rows_per_band(int W, int H, int tracer, bool stream);
// fp32 handles: float64 host arrays <-> the device state through a float64 staging buffer; M slabs of n elements,
// `pitch` elements apart on the device and n apart in the staging buffer
void launch_narrow(float *dst, long pitch, const double *src, long n, int M, hipStream_t s);
void launch_widen(double *dst, const float *src, long pitch, long n, int M, hipStream_t s);

// GCM_PE2D: one Euler stage; base/stage/out are {p,u,v,t,q} interior pointers (wrap only)
void launch_pe2d_stage(const double *const base[5], const double *const stage[5], double *const out[5],
                       const double *exner_tab, int W, int H, double dt, double dx, hipStream_t s);

// fills tab[256] (host) for gcm_math.h's exner(); kappa and P0 as in constants.py:28,31
void build_exner_table(double *tab);

// ghost rows for a single band that is stepped with wrap_j == 0 (tests) and halo pack/unpack
template <typename T> void launch_copy_rows(T *dst, const T *src, int W, int nrows, hipStream_t s);

// up to 5 contiguous segments copied by ONE launch (ghost-row pack / unpack of all fields)
struct SegCopy {          // up to (5 fields + the ground temperature + GCM_MAX_TRACERS tracers) x 2 sides in one launch
    double *dst[44];
    const double *src[44];
    long n[44];
    int nseg;
};
// stop: an event signalled by the copy kernel's own completion (hipExtLaunchKernelGGL), or null
void launch_seg_copy(const SegCopy &c, hipStream_t s, hipEvent_t stop = nullptr);

}  // namespace gcm

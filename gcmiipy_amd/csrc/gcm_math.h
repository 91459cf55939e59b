// Device arithmetic shared by the staged and the fused kernels, so that the two
// variants give bit-identical results (tests compare them at full size).
//
// Expression order follows the reference (file:line at each function).  Allowed
// departures, all far inside the 1e-10 relative tolerance (they move results by
// O(1e-16) relative): division by a loop-invariant scalar is a multiply by its
// host-computed reciprocal; x / y per cell is x * rcp(y) with two Newton steps;
// (P0/p)**kappa is exp(kappa * (log P0 - log p)); hipcc contracts a*b+c to fma.
#pragma once
#include <hip/hip_runtime.h>

#include "sw2d_kernels.h"

namespace gcm {

constexpr double kG = 9.8;                    // constants.py:45
constexpr double kRd = 287.0;                 // constants.py:16
constexpr double kRv = 461.0;                 // constants.py:78
constexpr double kCp = 1004.0;                // constants.py:22
constexpr double kKappa = 287.0 / 1004.0;     // constants.py:28
constexpr double kP0 = 100000.0;              // constants.py:31
constexpr double kMuAir = 18.5 * 1e-6;        // constants.py:51

// 1/x: v_rcp_f64 seed + two Newton-Raphson steps, no denormal/inf fix-ups.  Most operands on this path are
// pressures, densities and sigma thicknesses, far from either end of the range.  Two callers are not: the limiter
// weights of face_flux (below) and of tracer_face (pe25d_tracer_lim.h) take the reciprocal of a sum of tracer
// differences, which on the flank of a compact tracer blob is a denormal.  Measured on an MI355X: for x <= 2^-1024,
// where 1/x overflows, the result is NaN (the seed is an infinity, the Newton steps take it to NaN); v_rcp_f32
// returns an infinity for EVERY denormal x (profiles/tracer_range/).  face_flux at fp64 limits a face only where both
// differences are normal numbers, so that their sum has a finite reciprocal; face_flux at fp32 and tracer_face clamp
// the product to the weight's range, which takes NaN and infinity to its upper end.  Below the smallest normal number
// either choice moves the result by less than that number (tests/tracer_range_cases.py).
__device__ __forceinline__ double rcp(double x) {
    double r = __builtin_amdgcn_rcp(x);
    double e = __builtin_fma(-x, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-x, r, 1.0);
    r = __builtin_fma(r, e, r);
    return r;
}
// fp32: v_rcp_f32 is 1 ulp
__device__ __forceinline__ float rcp(float x) { return __builtin_amdgcn_rcpf(x); }
constexpr double kTinyF64 = 2.2250738585072014e-308;    // the smallest normal number: from it on 1/x is finite

// ---- (p / P0) ** kappa by table + short series --------------------------------------
// p = 2^e m, m in [1,2); i = top 6 mantissa bits; rc_i ~ 1/c_i with c_i the midpoint of
// the i-th sixty-fourth of [1,2); t = m rc_i - 1 exactly (fma), |t| <= 2^-7;
//   (p/P0)^kappa = [2^(kappa e) P0^-kappa] * [(1/rc_i)^kappa] * (1 + t)^kappa
// with the two bracketed factors from a 2 KB table (built in extended precision on the
// host, gcm_build_exner_table) and the last a degree-7 binomial series (truncation
// < 1e-18).  Max relative error vs extended precision 3e-16..5.3e-16 (tests/test_math_cpu.py);
// numpy's pow, which the reference uses, is at 1.5e-16.  Valid for 2^-64 <= p < 2^64;
// outside (or NaN / negative) the result is NaN, as pow gives for a negative base.
constexpr double kBinom1 = kKappa;
constexpr double kBinom2 = kBinom1 * (kKappa - 1) / 2;
constexpr double kBinom3 = kBinom2 * (kKappa - 2) / 3;
constexpr double kBinom4 = kBinom3 * (kKappa - 3) / 4;
constexpr double kBinom5 = kBinom4 * (kKappa - 4) / 5;
constexpr double kBinom6 = kBinom5 * (kKappa - 5) / 6;
constexpr double kBinom7 = kBinom6 * (kKappa - 6) / 7;

// One routine for the device and the host (the host probes of the phases that call it, e.g. gcm_boundary_layer_surface):
// only how the bits of p are taken apart and m is put together differs, every operation on them is the same.
__host__ __device__ __forceinline__ double exner(double p, const double *tab /* device: LDS */) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int hi = __double2hiint(p);
    const int e = ((hi >> 20) & 0x7ff) - 1023;
    const int idx = (hi >> 14) & 63;
    const double m = __hiloint2double((hi & 0x000fffff) | 0x3ff00000, __double2loint(p));
    const int ec = min(max(e, -64), 63);
#else
    unsigned long long bits;
    __builtin_memcpy(&bits, &p, sizeof bits);
    const int hi = (int)(unsigned)(bits >> 32);
    const int e = ((hi >> 20) & 0x7ff) - 1023;
    const int idx = (hi >> 14) & 63;
    const unsigned long long mbits = ((unsigned long long)(unsigned)((hi & 0x000fffff) | 0x3ff00000) << 32) | (bits & 0xffffffffull);
    double m;
    __builtin_memcpy(&m, &mbits, sizeof m);
    const int ec = e < -64 ? -64 : (e > 63 ? 63 : e);
#endif
    const double E = tab[ec + 64];
    const double rc = tab[128 + 2 * idx], ck = tab[129 + 2 * idx];
    const double t = __builtin_fma(m, rc, -1.0);
    // Estrin: 1 + t (b1 + t b2) + t^3 [(b3 + t b4) + t^2 (b5 + t b6) + t^4 b7]
    const double t2 = t * t, t4 = t2 * t2;
    const double q12 = __builtin_fma(t, kBinom2, kBinom1);
    const double q34 = __builtin_fma(t, kBinom4, kBinom3);
    const double q56 = __builtin_fma(t, kBinom6, kBinom5);
    const double hi3 = __builtin_fma(t4, kBinom7, __builtin_fma(t2, q56, q34));
    const double poly = __builtin_fma(t * t2, hi3, __builtin_fma(t, q12, 1.0));
    const double r = E * ck * poly;
    const bool ok = (hi >= 0) && (e >= -64) && (e <= 63);   // hi >= 0: sign bit clear
    return ok ? r : __builtin_nan("");
}
// fp32: the float64 table + series, rounded to float once.  (__powf expands to ~110 VALU instructions -- the fp32
// kernels executed TWICE the vector instructions of the fp64 ones -- and is less accurate than one rounding.)
__device__ __forceinline__ float exner(float p, const double *tab) { return (float)exner((double)p, tab); }

// value of the wave's lane-1 / lane+1 (columns i-1 / i+1): wave64 DPP shifts,
// two v_mov_b32_dpp per double, no LDS.  Lane 0 / 63 read 0 (bound_ctrl; no tied
// `old` operand, so no register copy) -- those lanes are halo and never stored.
__device__ __forceinline__ double from_west(double x) {
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x138 /*wave_shr:1*/, 0xf, 0xf, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x138, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double from_east(double x) {
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x130 /*wave_shl:1*/, 0xf, 0xf, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x130, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
// fp32 flavours: one DPP move per value
__device__ __forceinline__ float from_west(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x138 /*wave_shr:1*/, 0xf, 0xf, true));
}
__device__ __forceinline__ float from_east(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x130 /*wave_shl:1*/, 0xf, 0xf, true));
}
// fp32 with two columns per lane (the 120-column strip of sw2d_fused_kernel): lane L of a strip holds columns
// 2L and 2L+1 as one vector, so that a row segment is one 8-byte request per lane.  Arithmetic on the vector is
// elementwise (v_pk_* instructions); the helpers below apply the scalar ones per column.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 rcp(f32x2 x) { return f32x2{rcp(x.x), rcp(x.y)}; }
__device__ __forceinline__ f32x2 exner(f32x2 p, const double *tab) { return f32x2{exner(p.x, tab), exner(p.y, tab)}; }
// the column west of each: the west lane's second column, then the lane's own first; east likewise
__device__ __forceinline__ f32x2 from_west(f32x2 x) { return f32x2{from_west(x.y), x.x}; }
__device__ __forceinline__ f32x2 from_east(f32x2 x) { return f32x2{x.y, from_east(x.x)}; }
// the word that holds the sign bit
__device__ __forceinline__ int sign_word(double x) { return __double2hiint(x); }
__device__ __forceinline__ int sign_word(float x) { return __float_as_int(x); }

// ---- 2-D shallow water operators (matsuno_c_grid.py) -------------------------
// names: c=(j,i) w=(j,i-1) e=(j,i+1) n=(j-1,i) s=(j+1,i) sw=(j+1,i-1)

// advection_of_velocity_u, matsuno_c_grid.py:15-51
template <typename T>
__device__ __forceinline__ T adv_vel_u(T uc, T uw, T ue, T un, T us, T vc, T vw, T vs, T vsw, T h_dx) {
    // the reference's (a + b) / 2 factors are exact, so they are folded into h_dx = 0.5/dx
    T u_ipj = ue + uc, u_imj = uw + uc, v_ijm = vw + vc, v_ijp = vsw + vs;
    T du_ipj = ue - uc, du_imj = uc - uw, du_ijp = us - uc, du_ijm = uc - un;
    return (u_ipj * du_ipj + u_imj * du_imj + v_ijp * du_ijp + v_ijm * du_ijm) * h_dx;
}

// advection_of_velocity_v, matsuno_c_grid.py:54-80
template <typename T>
__device__ __forceinline__ T adv_vel_v(T vc, T vw, T ve, T vn, T vs, T uc, T un, T uw, T usw, T h_dx) {
    T v_ijp = vs + vc, v_ijm = vn + vc, u_ipj = uc + un, u_imj = uw + usw;
    T dv_ipj = ve - vc, dv_imj = vc - vw, dv_ijp = vs - vc, dv_ijm = vc - vn;
    return (u_ipj * dv_ipj + u_imj * dv_imj + v_ijp * dv_ijp + v_ijm * dv_ijm) * h_dx;
}

// geopotential_gradient_u / _v, matsuno_c_grid.py:97-106: (p[+1] - p) / dx * G
template <typename T>
__device__ __forceinline__ T geo_grad(T p_next, T pc, T g_dx) {
    return (p_next - pc) * g_dx;          // g_dx = G / dx folded on the host
}

// advection_of_geopotential, matsuno_c_grid.py:109-118
template <typename T>
__device__ __forceinline__ T adv_geo(T uc, T uw, T vc, T vn, T pc, T pw, T pe, T pn, T ps, T h_dx) {
    T up_imj = (pw + pc) * uw;
    T up_ipj = (pe + pc) * uc;
    T vp_ijm = (pn + pc) * vn;
    T vp_ijp = (ps + pc) * vc;
    return (up_ipj - up_imj) * h_dx + (vp_ijp - vp_ijm) * h_dx;
}

// finite_laplacian_2d * mu, viscosity.py:12-25
template <typename T>
__device__ __forceinline__ T visc_u(T uc, T uw, T ue, T un, T us, T mu_dx2) {
    T top = us + un + ue + uw - T(4.0) * uc;
    return top * mu_dx2;                   // mu_dx2 = mu_air / dx^2 folded on the host
}

// density_from + geopotential_from + scaling, matsumo_temp.py:13-19,28-30,45-47.
// Returns Rd T / p (= Rd / (rho Rd) ... i.e. 1/rho), geo = p/(G rho) and the mass-weighted
// theta p t.  Two constant factors are folded away: the reference's scaling/unscaling by
// dx*dx (matsumo_temp.py:28-35) cancels exactly in  t* = (p t dx^2 - dt adv(p t dx^2)) /
// (p* dx^2)  because adv() is linear, and Rd of 1/rho = Rd T / p is carried by the viscosity
// constant (mu Rd / dx^2).  Both move results by O(1 ulp).
// The table is float64 for either real type (exner()).
template <typename T>
struct Thermo { T t_over_p, geo, st; };
template <typename T>
__device__ __forceinline__ Thermo<T> thermo(T p, T t, const double *tab, T rcp_p) {
    T temp = t * exner(p, tab);           // t / (1e5/p)**kappa
    Thermo<T> r;
    r.t_over_p = temp * rcp_p;                 // 1/rho = Rd * (T / p)
    r.geo = temp * T(kRd / kG);                // p / (G rho) = Rd T / G
    r.st = p * t;
    return r;
}
template <typename T>
__device__ __forceinline__ Thermo<T> thermo(T p, T t, const double *tab) {
    return thermo(p, t, tab, rcp(p));
}

// ---- tracer face flux (two_d.py:103-116,135-149; flux_limiter.py:10-27) -----------
// flux through the face between cells 0 and +1 along an axis, times dt/dx.
template <bool LIMIT, typename T>
__device__ __forceinline__ T face_flux(T vel, T qm1, T q0, T q1, T q2, T dtdx) {
    const bool pos = vel > T(0.0);                      // strict >, as flux_limiter.py:24
    // (q0 max(vel,0) + q1 min(vel,0)) dt/dx: one of the two products is a zero
    const T vd = vel * dtdx;
    const T f_low = (pos ? q0 : q1) * vd;
    if (!LIMIT) return f_low;
    const T f_high = vd * ((q0 + q1) * T(0.5));
    const T b = q1 - q0;
    const T num = pos ? q0 - qm1 : q2 - q1;
    // van_leer(r), r = num / b (0 where b == 0, flux_limiter.py:19):
    // (r + |r|) / (1 + |r|) = 2 |num| / (|b| + |num|) if num b > 0 else 0 -- one reciprocal
    const T an = fabs(num), ab = fabs(b);
    // r > 0 <=> num and b are nonzero with equal signs (sign bits compared: no underflow)
    const bool same = (sign_word(num) ^ sign_word(b)) >= 0;
    // 0 < phi < 2, and a sum of denormals has no reciprocal here (rcp above).  Either guard leaves the bits of every
    // face with normal differences as they were; each type takes the one that keeps its fused kernels' registers
    // (profiles/tracer_range/): a clamp costs the fp64 row march 0.2-0.3 % of c3, the comparisons cost the fp32
    // one-column kernel 5 VGPRs and a wave.
    T phi;
    if constexpr (sizeof(T) == 8) {
        // "nonzero" taken as "a normal number": a face with a denormal difference is donor-cell -- what the weight
        // would have multiplied is smaller than the smallest normal number.  The comparisons stand where `> 0` stood.
        phi = same && an >= kTinyF64 && ab >= kTinyF64 ? (an + an) * rcp(ab + an) : T(0.0);
    } else {
        // the clamp of tracer_face (pe25d_tracer_lim.h): the infinity of v_rcp_f32 goes to the weight's upper end
        phi = same && an > T(0.0) && ab > T(0.0) ? fmin((an + an) * rcp(ab + an), T(2.0)) : T(0.0);
    }
    return f_low + phi * (f_high - f_low);
}
template <bool LIMIT>
__device__ __forceinline__ f32x2 face_flux(f32x2 vel, f32x2 qm1, f32x2 q0, f32x2 q1, f32x2 q2, f32x2 dtdx) {
    return f32x2{face_flux<LIMIT>(vel.x, qm1.x, q0.x, q1.x, q2.x, dtdx.x),
                 face_flux<LIMIT>(vel.y, qm1.y, q0.y, q1.y, q2.y, dtdx.y)};
}

}  // namespace gcm

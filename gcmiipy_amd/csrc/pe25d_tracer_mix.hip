// GCM_PE25D, implicit vertical mixing of the passive tracers (gcm_set_tracer_mixing): backward-Euler diffusion of the
// mixing ratio in sigma with zero flux at the top and the bottom, one launch right behind each corrector launch of the
// tracer kernel and in front of the forcing's, over the same rows, for the mixed tracers only.
//
//   coefficients (host, float64; gcm_tracer_mixing_coeffs), K[m] the diffusivity between levels m and m + 1:
//     a[-1] = a[L-1] = 0;   a[m] = dtd * K[m] / (0.5 * (dsig[m] + dsig[m+1]))
//     lo[k] = a[k-1] / dsig[k];   up[k] = a[k] / dsig[k];   d = 1.0 + lo[k] + up[k]
//     w[0]  = 1.0 / d;            w[k] = 1.0 / (d - lo[k] * g[k-1])   (k >= 1);      g[k] = up[k] * w[k]
//   the solve of one column (device, in T, lo / w / g rounded to T):
//     y[0] = c[0] * w[0];       y[k] = (c[k] + lo[k] * y[k-1]) * w[k]     k = 1 .. L-1
//     x[L-1] = y[L-1];          x[k] = y[k] + g[k] * x[k+1]               k = L-2 .. 0;       c = x
//
// Every operation is rounded on its own: contraction is off for the whole file (the Makefile builds it with
// -ffp-contract=fast-honor-pragmas), host and device, so a NumPy restatement gives the same bits.  All coefficients
// are >= 0: a non-negative column stays non-negative.  Pinned cells (gcm_set_tracer_forcing) are NOT boundary
// conditions of the solve: the forcing that follows sets them again.
//
// The tracers' layout is [j][k][i]: one lane owns one column (j, i), a wave is 64 consecutive i of one row, so the
// request of a level is one contiguous run.  Addresses are a wave-uniform base (entry, row, level) plus one 32-bit
// byte offset per lane, as in pe25d_tracer.h.  The coefficient tables are wave-uniform: they are read from the
// constant address space, through scalar loads, and cost no vector register per level.  With L <= LMAX the column
// stays in registers between the two sweeps: one read and one write of each cell.
#pragma clang fp contract(off)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "pe25d_tracer_mix.h"

namespace gcm {

// ---------------------------------------------------------------- the coefficients (host)
int tracer_mixing_coeffs(int L, const double *dsig, const double *k, double dtd, double *lo, double *w, double *g, std::string *err) {
    if (L < 2) { *err = "gcm_tracer_mixing_coeffs: L must be 2 or more (one level has no interface to mix across)"; return GCM_ERR_ARG; }
    if (!dsig || !k || !lo || !w || !g) { *err = "gcm_tracer_mixing_coeffs: a null pointer"; return GCM_ERR_ARG; }
    for (int m = 0; m < L - 1; ++m)
        if (!std::isfinite(k[m]) || k[m] < 0.0) {
            *err = "gcm_tracer_mixing_coeffs: K must be finite and >= 0 at every interface";
            return GCM_ERR_ARG;
        }
    // a[m]: the interface between levels m and m + 1; none above level 0 or below level L - 1
    const auto a = [&](int m) {
        if (m < 0 || m >= L - 1) return 0.0;
        const double num = dtd * k[m];
        const double sum = dsig[m] + dsig[m + 1];
        const double den = 0.5 * sum;
        return num / den;
    };
    for (int i = 0; i < L; ++i) {
        const double lo_k = a(i - 1) / dsig[i];
        const double up_k = a(i) / dsig[i];
        const double d1 = 1.0 + lo_k;
        const double d = d1 + up_k;
        double w_k;
        if (i == 0) {
            w_k = 1.0 / d;
        } else {
            const double t = lo_k * g[i - 1];
            const double den = d - t;
            w_k = 1.0 / den;
        }
        lo[i] = lo_k;
        w[i] = w_k;
        g[i] = up_k * w_k;
    }
    return GCM_OK;
}

// ---------------------------------------------------------------- the solve (device)
constexpr int kTmThreads = 256;
constexpr int kTmWaves = kTmThreads / 64;

#define TM_GLOBAL __attribute__((address_space(1)))
#define TM_CONST __attribute__((address_space(4)))

// a wave-uniform address through an opaque scalar register pair (pe25d_tracer.h's sbase): the request is then the
// scalar base + the lane's 32-bit offset, not a 64-bit address per lane
__device__ inline TM_GLOBAL char *tm_sbase(const void *p) {
    unsigned long long v = (unsigned long long)p;
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
    lo = __builtin_amdgcn_readfirstlane(lo);
    hi = __builtin_amdgcn_readfirstlane(hi);
    asm volatile("" : "+s"(lo), "+s"(hi));
    return (TM_GLOBAL char *)(((unsigned long long)hi << 32) | lo);
}

// grid (workgroups, entries); a wave takes 64 columns of one row.  LMAX > 0: L <= LMAX and y stays in registers
// (loops unrolled over LMAX); LMAX == 0: any L, y parked in c itself
template <typename T, int LMAX>
__global__ __launch_bounds__(kTmThreads) void pe_tracer_mix_kernel(TracerMixArgsT<T> a) {
    const int W = a.W, L = a.L;
    const int tiles = (W + 63) / 64;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));
    const unsigned item = (unsigned)blockIdx.x * kTmWaves + (unsigned)wave;   // (row of the launch, tile of 64 columns)
    if (item >= (unsigned)(a.n0 + a.n1) * (unsigned)tiles) return;
    // (the quotient comes out of the vector unit: back to a scalar register, and every address below is scalar arithmetic)
    const int r = __builtin_amdgcn_readfirstlane((int)(item / (unsigned)tiles)), ct = (int)(item - (unsigned)r * (unsigned)tiles);
    const int j = r < a.n0 ? a.j0 + r : a.jb0 + (r - a.n0);
    const int i = ct * 64 + (int)(threadIdx.x % 64);
    if (i >= W) return;
    T *const col = a.c[blockIdx.y] + (long)j * L * W;            // level 0 of row j (wave-uniform)
    const TM_CONST T *const lo = (const TM_CONST T *)a.tab + (long)blockIdx.y * 3 * L;
    const TM_CONST T *const w = lo + L, *const g = w + L;
    const unsigned ol = (unsigned)i * (unsigned)sizeof(T);
    // (the lane offset is made opaque at every request, so that its widening stays in the request's own block and the
    // request keeps the form scalar base + 32-bit lane offset)
    const auto ld = [&](int k) {
        unsigned o = ol;
        asm volatile("" : "+v"(o));
        return *(const TM_GLOBAL T *)(tm_sbase(col + (long)k * W) + o);
    };
    const auto st = [&](int k, T v) {
        unsigned o = ol;
        asm volatile("" : "+v"(o));
        *(TM_GLOBAL T *)(tm_sbase(col + (long)k * W) + o) = v;
    };

    if (LMAX > 0) {
        // the whole column is requested before any of it is used (one memory latency per column, not per level)
        // (no early exit: the loops unroll to static registers.  Each sweep compares with a copy of L of its own, else
        // the compiler keeps the 3 x LMAX outcomes of k < L alive as lane masks, more than there are scalar registers)
        int Ll = L, Lu = L, Ld = L;
        asm volatile("" : "+s"(Ll), "+s"(Lu), "+s"(Ld));
        T y[LMAX > 0 ? LMAX : 1];
#pragma unroll
        for (int k = 0; k < LMAX; ++k) {
            if (k < Ll) y[k] = ld(k);
        }
        y[0] = y[0] * w[0];
#pragma unroll
        for (int k = 1; k < LMAX; ++k) {
            if (k < Lu) {
                const T t = lo[k] * y[k - 1];
                const T s = y[k] + t;
                y[k] = s * w[k];
            }
        }
        T x = T(0);
#pragma unroll
        for (int k = LMAX - 1; k >= 0; --k) {
            if (k >= Ld) continue;
            if (k == Ld - 1) {
                x = y[k];
            } else {
                const T t = g[k] * x;
                x = y[k] + t;
            }
            st(k, x);
        }
    } else {
        T y = ld(0) * w[0];
        st(0, y);
        for (int k = 1; k < L; ++k) {
            const T t = lo[k] * y;
            const T s = ld(k) + t;
            y = s * w[k];
            st(k, y);
        }
        T x = y;                                                 // (x[L-1] = y[L-1]: in place already)
        for (int k = L - 2; k >= 0; --k) {
            const T t = g[k] * x;
            x = ld(k) + t;
            st(k, x);
        }
    }
}

template <typename T>
void launch_tracer_mix(const TracerMixArgsT<T> &a, int entries, hipStream_t s) {
    const long rows = (long)a.n0 + a.n1;
    if (entries <= 0 || rows <= 0 || a.L < 2) return;
    const long items = rows * ((a.W + 63) / 64);
    const dim3 grid((unsigned)((items + kTmWaves - 1) / kTmWaves), (unsigned)entries), block(kTmThreads);
    static_assert(kTmLevelsMax == 40, "the largest instantiation below");
    if (a.L <= 24) hipLaunchKernelGGL((pe_tracer_mix_kernel<T, 24>), grid, block, 0, s, a);
    else if (a.L <= 40) hipLaunchKernelGGL((pe_tracer_mix_kernel<T, 40>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((pe_tracer_mix_kernel<T, 0>), grid, block, 0, s, a);
}

template void launch_tracer_mix<double>(const TracerMixArgsT<double> &, int, hipStream_t);
template void launch_tracer_mix<float>(const TracerMixArgsT<float> &, int, hipStream_t);

// ---------------------------------------------------------------- the tables' way to the device
template <typename T>
struct TmFillArgsT {
    T v[kTmFillMax];
    T *dst;
    int n;
};

template <typename T>
__global__ __launch_bounds__(kTmFillMax) void pe_tracer_mix_fill_kernel(TmFillArgsT<T> a) {
    const int t = (int)threadIdx.x;
    if (t < a.n) a.dst[t] = a.v[t];
}

template <typename T>
void launch_tracer_mix_fill(T *dst, const T *values, int n, hipStream_t s) {
    if (n <= 0) return;
    TmFillArgsT<T> a{};
    a.n = std::min(n, kTmFillMax);
    std::copy(values, values + a.n, a.v);
    a.dst = dst;
    hipLaunchKernelGGL(pe_tracer_mix_fill_kernel<T>, dim3(1), dim3(kTmFillMax), 0, s, a);
}

template void launch_tracer_mix_fill<double>(double *, const double *, int, hipStream_t);
template void launch_tracer_mix_fill<float>(float *, const float *, int, hipStream_t);

}  // namespace gcm

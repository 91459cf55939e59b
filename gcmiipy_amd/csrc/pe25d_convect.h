// GCM_PE25D, what the convective adjustment (pe25d_convect.hip) and the tracers' convective mixing
// (pe25d_convect_tracers.hip) share: the pooling routine, the neutral profile's factor, the block stacks of the host and
// of a wave, and the constants of the two kernels' common shape.  Both units switch contraction off for the whole file
// ahead of this header (#pragma clang fp contract(off), -ffp-contract=fast-honor-pragmas): a column's blocks are the
// same bits in either kernel and on the host.
#pragma once
#include "pe25d_host.h"

namespace gcm {

// ---------------------------------------------------------------- the pooling (host and device: one routine)
// A stack `St` offers S, Wt, Qs, D, val (double &) and n (int &) of slot b; `top` blocks are on it.  The new level's
// block is kept in registers while it absorbs the blocks below it and is stored once.  -> the new number of blocks
template <class St>
__host__ __device__ inline int convect_push(St &st, int top, double y, double w, double q, double d) {
    double S = w * y, Wt = w, Qs = q * d, D = d, val = y;
    int n = 1;
    while (top > 0 && val < st.val(top - 1)) {
        --top;
        S = st.S(top) + S;
        Wt = st.Wt(top) + Wt;
        Qs = st.Qs(top) + Qs;
        D = st.D(top) + D;
        n = st.n(top) + n;
        val = S / Wt;
    }
    st.S(top) = S; st.Wt(top) = Wt; st.Qs(top) = Qs; st.D(top) = D; st.val(top) = val; st.n(top) = n;
    return top + 1;
}

// the neutral profile's factor r and the compared value y of a cell; dry: r = 1 and y = theta, no operation on it
__host__ __device__ inline double convect_r(double p_lev, double kdiff) { return exp(kdiff * log(p_lev / kP0)); }

struct CvHostStack {
    std::vector<double> s, wt, qs, d, v;
    std::vector<int> c;
    explicit CvHostStack(int L) : s(L), wt(L), qs(L), d(L), v(L), c(L) {}
    double &S(int b) { return s[b]; }
    double &Wt(int b) { return wt[b]; }
    double &Qs(int b) { return qs[b]; }
    double &D(int b) { return d[b]; }
    double &val(int b) { return v[b]; }
    int &n(int b) { return c[b]; }
};

// ---------------------------------------------------------------- the kernels' common shape
constexpr int kCvThreads = 64;       // one wave: the workgroup's LDS is that wave's stack
constexpr int kCvBatch = 8;          // levels requested together in pass 1, then compared in order
constexpr int kCvBatch2 = 4;         // levels requested together in pass 2, then pushed in order
constexpr size_t kCvSlotBytes = 5 * sizeof(double) + sizeof(int);

constexpr size_t kCvLdsCap = 160 * 1024;   // a workgroup's LDS on gfx950, the figure pe25d_create sizes its kernels by

size_t convect_lds_bytes(int L);     // the Exner table and the wave's stack (pe25d_convect.hip)

// the lane's stack in LDS: slot b of array a at base[(a L + b) 64 + lane]
struct CvLdsStack {
    double *base;
    int *cnt;
    int L;
    __host__ __device__ double &at(int a, int b) { return base[(a * L + b) * kCvThreads]; }
    __host__ __device__ double &S(int b) { return at(0, b); }
    __host__ __device__ double &Wt(int b) { return at(1, b); }
    __host__ __device__ double &Qs(int b) { return at(2, b); }
    __host__ __device__ double &D(int b) { return at(3, b); }
    __host__ __device__ double &val(int b) { return at(4, b); }
    __host__ __device__ int &n(int b) { return cnt[b * kCvThreads]; }
};

}  // namespace gcm

// GCM_PE25D, the device monitor of the passive tracers and q (gcm_tracer_stats): per field min, max,
// mass = sum c p dsig_k, air = sum p dsig_k, the cells < 0 and the NaN cells, over the handle's own rows.
//
// Each field is read once ([j][k][i] in the handle's real type, widened exactly), p once per row and column chunk;
// every product and sum is float64 on a float64 dsig table.  A 256-thread workgroup takes (row, 256-column chunk)
// units in steps of the grid; a lane keeps p of its column in a register while it walks the L levels, and a wave's
// request is one contiguous run of a level.  Nothing here is atomic: a lane adds in (unit, level) order, the 64
// lanes of a wave combine in a fixed butterfly, the four waves in wave order through LDS, and the second launch
// folds the workgroups' records in index order the same way -- the same state gives the same bits.
#include <algorithm>
#include <cmath>

#include "pe25d_tracer_stats.h"

namespace gcm {

constexpr int kTsThreads = 256;
constexpr int kTsWaves = kTsThreads / 64;
// the most workgroups PER FIELD (the grid is groups x fields: 17 x 1024 with 16 tracers and q): 720 x 1440 (C4) has
// 4320 units, so a workgroup there walks 4 or 5 of them; the 86 rows of an N = 8 band have 516, one each
constexpr int kTsGroupsMax = 1024;

int tracer_stats_groups(int H, int W) {
    const long units = (long)H * ((W + kTsThreads - 1) / kTsThreads);
    return (int)std::min<long>(units, kTsGroupsMax);
}

// min and max skip NaN (fmin / fmax); the NaN count restores np.min / np.max's answer at the very end.
// The counts are exact in double far beyond any field's size
struct TsRec {
    double mn, mx, mass, air, neg, nan;
};

__device__ inline void ts_merge(TsRec &r, const TsRec &o) {
    r.mn = fmin(r.mn, o.mn);
    r.mx = fmax(r.mx, o.mx);
    r.mass += o.mass;
    r.air += o.air;
    r.neg += o.neg;
    r.nan += o.nan;
}

// the workgroup's record, valid in thread 0.  Every wave runs the same xor butterfly (both partners add the same
// two numbers, so all 64 lanes end on the same bits); thread 0 then takes the waves in order
__device__ inline void ts_block_reduce(TsRec &r) {
    __shared__ TsRec sh[kTsWaves];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        TsRec o;
        o.mn = __shfl_xor(r.mn, d, 64);
        o.mx = __shfl_xor(r.mx, d, 64);
        o.mass = __shfl_xor(r.mass, d, 64);
        o.air = __shfl_xor(r.air, d, 64);
        o.neg = __shfl_xor(r.neg, d, 64);
        o.nan = __shfl_xor(r.nan, d, 64);
        ts_merge(r, o);
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        r = sh[0];
        for (int w = 1; w < kTsWaves; ++w) ts_merge(r, sh[w]);
    }
}

__device__ inline void ts_store(double *dst, const TsRec &r) {
    dst[0] = r.mn; dst[1] = r.mx; dst[2] = r.mass; dst[3] = r.air; dst[4] = r.neg; dst[5] = r.nan;
}

// grid (groups, fields): blockIdx.y = the field, q after the tracers.  air is summed by field 0's workgroups only
template <typename T>
__global__ __launch_bounds__(kTsThreads) void pe_tracer_stats_kernel(TracerStatsArgs a) {
    const int f = (int)blockIdx.y;
    const T *c = f < a.ntr ? (const T *)a.tr + (long)f * a.tstride : (const T *)a.q;
    const T *p = (const T *)a.p;
    const bool with_air = f == 0;
    const int W = a.W, L = a.L;
    const int ncol = (W + kTsThreads - 1) / kTsThreads, units = a.H * ncol;
    TsRec r{INFINITY, -INFINITY, 0.0, 0.0, 0.0, 0.0};
    unsigned neg = 0, nnan = 0;
    for (int u = (int)blockIdx.x; u < units; u += (int)gridDim.x) {
        const int j = u / ncol, i = (u - j * ncol) * kTsThreads + (int)threadIdx.x;
        if (i >= W) continue;                                  // (no barrier inside the loop)
        const double pc = (double)p[(long)j * W + i];
        const T *cj = c + (long)j * L * W + i;
#pragma unroll 4
        for (int k = 0; k < L; ++k) {
            const double x = (double)cj[(long)k * W];
            const double w = pc * a.dsig[k];
            r.mn = fmin(r.mn, x);
            r.mx = fmax(r.mx, x);
            r.mass += x * w;
            if (with_air) r.air += w;
            neg += x < 0.0 ? 1u : 0u;
            nnan += x != x ? 1u : 0u;
        }
    }
    r.neg = (double)neg;
    r.nan = (double)nnan;
    ts_block_reduce(r);
    if (threadIdx.x == 0) ts_store(a.part + ((long)f * gridDim.x + blockIdx.x) * GCM_TRACER_STATS_WORDS, r);
}

// one workgroup per field: thread t folds records t, t + 256, ... in that order, then the workgroup as above.
// Every field's air is field 0's
__global__ __launch_bounds__(kTsThreads) void pe_tracer_stats_fold_kernel(TracerStatsArgs a, int groups) {
    const int f = (int)blockIdx.x;
    const double *own = a.part + (long)f * groups * GCM_TRACER_STATS_WORDS;
    TsRec r{INFINITY, -INFINITY, 0.0, 0.0, 0.0, 0.0};
    for (int b = (int)threadIdx.x; b < groups; b += kTsThreads) {
        const double *o = own + (long)b * GCM_TRACER_STATS_WORDS;
        const TsRec x{o[0], o[1], o[2], a.part[(long)b * GCM_TRACER_STATS_WORDS + 3], o[4], o[5]};
        ts_merge(r, x);
    }
    ts_block_reduce(r);
    if (threadIdx.x == 0) {
        if (r.nan > 0.0) r.mn = r.mx = NAN;                    // np.min / np.max propagate NaN
        ts_store(a.out + (long)f * GCM_TRACER_STATS_WORDS, r);
    }
}

template __global__ void pe_tracer_stats_kernel<double>(TracerStatsArgs);
template __global__ void pe_tracer_stats_kernel<float>(TracerStatsArgs);

void launch_tracer_stats(const TracerStatsArgs &a, bool f32, hipStream_t s) {
    const int groups = tracer_stats_groups(a.H, a.W);
    const dim3 grid((unsigned)groups, (unsigned)a.nf);
    if (f32) hipLaunchKernelGGL(pe_tracer_stats_kernel<float>, grid, dim3(kTsThreads), 0, s, a);
    else hipLaunchKernelGGL(pe_tracer_stats_kernel<double>, grid, dim3(kTsThreads), 0, s, a);
    hipLaunchKernelGGL(pe_tracer_stats_fold_kernel, dim3((unsigned)a.nf), dim3(kTsThreads), 0, s, a, groups);
}

}  // namespace gcm

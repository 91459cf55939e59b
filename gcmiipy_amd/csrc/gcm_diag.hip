// Diagnostics of libgcmcore.so: the two reduction kernels, gcm_diag / gcm_diag_members on a handle's current state,
// gcm_array_stats on a host array, and the GCM_PE25D records gcm_energy / gcm_stats.
#include <cmath>

#include "gcm_handle.h"

using namespace gcm;

// Both reductions are segmented: blockIdx.y picks a segment (an ensemble member) that starts `seg` elements
// after the previous one, and block (x, y) writes partial 4 * (y * gridDim.x + x).
template <typename T>
__global__ __launch_bounds__(256) void diag_kernel(const T *x, long n, double *out, long seg = 0) {
    // out[4*b + {0,1,2,3}] = max, min, sum, nan-count of this block's grid-stride share
    x += blockIdx.y * seg;
    out += 4 * (long)blockIdx.y * gridDim.x;
    double mx = -INFINITY, mn = INFINITY, sm = 0.0, nn = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const double v = (double)x[i];
        if (v != v) nn += 1.0;
        mx = fmax(mx, v);
        mn = fmin(mn, v);
        sm += v;
    }
    for (int o = 32; o > 0; o >>= 1) {
        mx = fmax(mx, __shfl_down(mx, o));
        mn = fmin(mn, __shfl_down(mn, o));
        sm += __shfl_down(sm, o);
        nn += __shfl_down(nn, o);
    }
    __shared__ double s[4][4];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s[w][0] = mx;
        s[w][1] = mn;
        s[w][2] = sm;
        s[w][3] = nn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) {
            s[0][0] = fmax(s[0][0], s[k][0]);
            s[0][1] = fmin(s[0][1], s[k][1]);
            s[0][2] += s[k][2];
            s[0][3] += s[k][3];
        }
        for (int k = 0; k < 4; ++k) out[4 * blockIdx.x + k] = s[0][k];
    }
}

// get_total_variation (constants.py:105-108): sum |x - roll(x, -1, axis)| for an array viewed as
// [n_outer][n_axis][n_inner]; wrap == 0: the slab after the last one (a band's south ghost row) is
// differenced instead of slab 0.  out[4*b + 2] = the block's partial sum, [3] = its NaN count.
template <typename T>
__global__ __launch_bounds__(256) void tv_kernel(const T *x, long n_outer, long n_axis, long n_inner, int wrap, double *out,
                                                 long seg = 0) {
    x += blockIdx.y * seg;
    out += 4 * (long)blockIdx.y * gridDim.x;
    const long n = n_outer * n_axis * n_inner;
    double sm = 0.0, nn = 0.0;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        const long i = e % n_inner, r = e / n_inner;
        const long a = r % n_axis, o = r / n_axis;
        const long an = (a + 1 == n_axis && wrap) ? 0 : a + 1;
        const double v = (double)x[e], w = (double)x[(o * n_axis + an) * n_inner + i];
        const double d = fabs(v - w);
        if (d != d) nn += 1.0;
        sm += d;
    }
    for (int o = 32; o > 0; o >>= 1) {
        sm += __shfl_down(sm, o);
        nn += __shfl_down(nn, o);
    }
    __shared__ double s[4][2];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s[w][0] = sm; s[w][1] = nn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[4 * blockIdx.x] = 0.0;
        out[4 * blockIdx.x + 1] = 0.0;
        out[4 * blockIdx.x + 2] = s[0][0] + s[1][0] + s[2][0] + s[3][0];
        out[4 * blockIdx.x + 3] = s[0][1] + s[1][1] + s[2][1] + s[3][1];
    }
}

// an array viewed as [n_outer][n_axis][n_inner] (see tv_kernel); the plain reduction takes all its elements
struct DiagShape {
    long n_outer, n_axis, n_inner;
    int wrap;
};

// One reduction launch, the kernel picked by (total variation or not, f32 or not): grid.x workgroups for each of
// grid.y segments `seg` elements apart; 4 doubles per workgroup to `out`.
static void launch_reduce(bool tv, bool f32, dim3 grid, const void *x, const DiagShape &sh, long seg, double *out, hipStream_t s) {
    const long n = sh.n_outer * sh.n_axis * sh.n_inner;
    const dim3 wg(256);
    if (tv && f32) hipLaunchKernelGGL(tv_kernel<float>, grid, wg, 0, s, (const float *)x, sh.n_outer, sh.n_axis, sh.n_inner, sh.wrap, out, seg);
    else if (tv) hipLaunchKernelGGL(tv_kernel<double>, grid, wg, 0, s, (const double *)x, sh.n_outer, sh.n_axis, sh.n_inner, sh.wrap, out, seg);
    else if (f32) hipLaunchKernelGGL(diag_kernel<float>, grid, wg, 0, s, (const float *)x, n, out, seg);
    else hipLaunchKernelGGL(diag_kernel<double>, grid, wg, 0, s, (const double *)x, n, out, seg);
}

// max, min, sum and NaN count, folded in the order the terms are handed over
struct Reduced {
    double mx = -INFINITY, mn = INFINITY, sm = 0.0, nn = 0.0;
    void add(double mx_, double mn_, double sm_, double nn_) {
        mx = std::fmax(mx, mx_);
        mn = std::fmin(mn, mn_);
        sm += sm_;
        nn += nn_;
    }
};

// the partials of nb workgroups, block 0 upwards
static Reduced fold(const double *part, int nb) {
    Reduced r;
    for (int b = 0; b < nb; ++b) r.add(part[4 * b], part[4 * b + 1], part[4 * b + 2], part[4 * b + 3]);
    return r;
}

// which field a gcm_diag_kind reduces, or a negative status
static int diag_field(gcm_handle *h, int kind) {
    switch (kind) {
        case GCM_DIAG_TV_P: case GCM_DIAG_TV_U: case GCM_DIAG_TV_V: case GCM_DIAG_TV_T: case GCM_DIAG_TV_Q:
            if (!h->has[kind - GCM_DIAG_TV_P]) return fail(h, GCM_ERR_ARG, "gcm_diag: the model has no such field");
            return kind - GCM_DIAG_TV_P;
        case GCM_DIAG_ANY_NAN: case GCM_DIAG_MAX_U: case GCM_DIAG_MIN_U: return GCM_U;
        case GCM_DIAG_MEAN_P: case GCM_DIAG_SUM_P: return GCM_P;
        case GCM_DIAG_MAX_V: case GCM_DIAG_MIN_V: return GCM_V;
        default: return fail(h, GCM_ERR_ARG, "gcm_diag: unknown kind");
    }
}

// a diagnostic's value from the reduced max, min, sum and NaN count of n elements
static double diag_value(int kind, const Reduced &r, double n) {
    switch (kind) {
        case GCM_DIAG_ANY_NAN: return r.nn > 0 ? 1.0 : 0.0;
        case GCM_DIAG_MAX_U: case GCM_DIAG_MAX_V: return r.nn > 0 ? NAN : r.mx;
        case GCM_DIAG_MIN_U: case GCM_DIAG_MIN_V: return r.nn > 0 ? NAN : r.mn;
        case GCM_DIAG_MEAN_P: return r.sm / n;
        case GCM_DIAG_SUM_P: return r.sm;
        default: return r.nn > 0 ? NAN : r.sm;             // total variation
    }
}

// A diagnostic of the current state by one launch and one synchronisation.  An ensemble handle (2-D, single band) reduces every
// member in a segment of its own (nb workgroups per member): per_member[M] (may be NULL) and / or *all, the figure over all members
// (a mean over all M H W cells; total variations add up, each member's rows wrapping inside the member).  The sums run per member
// first, block 0 upwards, then across members.
static int diag_run(gcm_handle *h, int kind, double *per_member, double *all) {
    const int f = diag_field(h, kind);
    if (f < 0) return f;
    const bool tv = kind >= GCM_DIAG_TV_P && kind <= GCM_DIAG_TV_Q;
    // a 2-D band differences its last row against the south ghost row: that row must belong to
    // the CURRENT state (bands exchange before a step, so after a step it is stale)
    if (tv && !h->pe && !h->wrap && !h->ghosts_current)
        return fail(h, GCM_ERR_STATE, "gcm_diag: total variation on a latitude band needs the current state's "
                                      "ghost rows (exchange them first: gcm_halo_pack2 / exchange / gcm_halo_unpack2)");
    const void *x = h->cur[f];
    int f32 = h->f32;
    long n = (long)h->H * h->W;
    DiagShape sh{1, h->H, h->W, h->wrap ? 1 : 0};
    if (h->pe) {
        x = pe25d_field(h->pe, f, &n, &f32);
        pe25d_tv_shape(h->pe, f, &sh.n_outer, &sh.n_axis, &sh.n_inner, &sh.wrap);
    }
    const int nb = diag_blocks_per_member(h), M = h->M;
    launch_reduce(tv, f32 != 0, dim3(nb, M), x, sh, M > 1 ? h->mstride : 0, h->diag_dev, h->stream);
    if (M > 1) HIPCHK(h, hipGetLastError());              // (one member: the last error stays with launch_status, as ever)
    std::vector<double> part(4 * (size_t)nb * M);
    HIPCHK(h, hipMemcpyAsync(part.data(), h->diag_dev, sizeof(double) * part.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    Reduced total;
    for (int m = 0; m < M; ++m) {
        const Reduced r = fold(&part[4 * (size_t)m * nb], nb);
        if (per_member) per_member[m] = diag_value(kind, r, (double)n);
        total.add(r.mx, r.mn, r.sm, r.nn);
    }
    if (all) *all = diag_value(kind, total, (double)n * M);
    return GCM_OK;
}

extern "C" {

int gcm_diag(gcm_handle *h, int kind, double *out) {
    if (!h || !out) return GCM_ERR_ARG;
    return diag_run(h, kind, nullptr, out);
}

int gcm_diag_members(gcm_handle *h, int kind, double *out, int n) {
    if (!h || !out) return GCM_ERR_ARG;
    if (n < h->M) return fail(h, GCM_ERR_ARG, "gcm_diag_members: out holds fewer values than the handle has members");
    return diag_run(h, kind, out, nullptr);
}

int gcm_energy(gcm_handle *h, const double *area, int area_len, double *out4) {
    if (!h || !area || !out4 || area_len < 1) return GCM_ERR_ARG;
    if (int rc = pe_only(h, "gcm_energy")) return rc;
    double o9[9];
    int rc = pe25d_stats(h->pe, area, area_len, o9, h->stream, &h->err);
    if (rc == GCM_OK) for (int q = 0; q < 4; ++q) out4[q] = o9[4 + q];
    return rc;
}

int gcm_stats(gcm_handle *h, const double *area, int area_len, double *out9) {
    if (!h || !area || !out9 || area_len < 1) return GCM_ERR_ARG;
    if (int rc = pe_only(h, "gcm_stats")) return rc;
    return pe25d_stats(h->pe, area, area_len, out9, h->stream, &h->err);
}

// constants.get_total_variation (constants.py:105-108) of ANY host array viewed as [n_axis][n_inner]
// (the roll is along axis 0), and the two reductions of constants.courant_number (:111-112), max and
// mean, for callers that hold no handle.  out3 = {sum |x - roll(x, -1, 0)|, max x, mean x}.
int gcm_array_stats(const double *x, long n_axis, long n_inner, double *out3) {
    if (!x || !out3 || n_axis < 1 || n_inner < 1) return GCM_ERR_ARG;
    if (gcm_device_count() < 1) {
        gcm_create_error() = "gcm_array_stats: no HIP device; no CPU fallback";
        return GCM_ERR_NODEVICE;
    }
    const long n = n_axis * n_inner;
    constexpr int nb = 256;
    const DiagShape sh{1, n_axis, n_inner, 1};
    double *dx = nullptr, *dp = nullptr;
    std::vector<double> part(8 * nb);
    hipError_t e = hipMalloc((void **)&dx, sizeof(double) * (size_t)n);
    if (e == hipSuccess) e = hipMalloc((void **)&dp, sizeof(double) * 8 * nb);
    if (e == hipSuccess) e = hipMemcpy(dx, x, sizeof(double) * (size_t)n, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch_reduce(true, false, dim3(nb), dx, sh, 0, dp, nullptr);
        launch_reduce(false, false, dim3(nb), dx, sh, 0, dp + 4 * nb, nullptr);
        e = hipMemcpy(part.data(), dp, sizeof(double) * 8 * nb, hipMemcpyDeviceToHost);
    }
    if (dx) (void)hipFree(dx);
    if (dp) (void)hipFree(dp);
    if (e != hipSuccess) {
        gcm_create_error() = std::string("gcm_array_stats: ") + hipGetErrorString(e);
        return GCM_ERR_HIP;
    }
    const Reduced tv = fold(part.data(), nb), r = fold(part.data() + 4 * nb, nb);
    // np.max propagates NaN (constants.py:111-112); fmax drops it, so the count decides
    out3[0] = tv.sm; out3[1] = r.nn > 0 ? NAN : r.mx; out3[2] = r.sm / (double)n;
    return GCM_OK;
}

}  // extern "C"

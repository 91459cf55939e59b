// GCM_PE25D, horizontal del-2 / del-4 diffusion of u, v, theta (and q) on sigma surfaces (gcm_set_hdiff, gcm_hdiff_step):
// one launch per application behind the Matsuno step and ahead of the solar step.  The contract: include/gcmcore.h.
//
//   tables (host, float64, every operation rounded on its own; gcm_hdiff_tables), j periodic:
//     s = nu dt (order 1) | sqrt(nu dt) (order 2);   ay = min(s / (dy dy), cmax)
//     centre rows (theta, q, u):  ax[j] = min(s / (dx_j[j] dx_j[j]), cmax);  area[j] = ((dx_h[j-1] + dx_h[j]) dy) 0.5
//                                 bs[j] = (ay (dx_h[j] dy)) / area[j];       bn[j] = (ay (dx_h[j-1] dy)) / area[j]
//     v rows:                     axv[j] = min(s / (dx_h[j] dx_h[j]), cmax); areav[j] = ((dx_j[j] + dx_j[j+1]) dy) 0.5
//                                 bsv[j] = (ay (dx_j[j+1] dy)) / areav[j];   bnv[j] = (ay (dx_j[j] dy)) / areav[j]
//   update (device, float64 for either storage type, rounded once to it; hdiff_cell, pe25d_hdiff.h), i and j periodic:
//     D(X) = ax[j] ((X[j][i+1] - X[j][i]) - (X[j][i] - X[j][i-1])) + (bs[j] (X[j+1][i] - X[j][i]) - bn[j] (X[j][i] - X[j-1][i]))
//     order 1: X' = X + D(X);   order 2: Y = D(X) kept in float64, X' = X - D(Y)
//
// What it is and is not: the operator acts level by level on the model's sigma surfaces, not on pressure surfaces, so
// over topography it mixes along the terrain-following levels; it acts component-wise on u and v, with no metric terms
// of the vector Laplacian (as incompressible_viscosity_2d does for the 2-D model); theta is not pressure-weighted, so
// sum area theta is conserved per level, not the mass-weighted sum; p and the passive tracers are not diffused (their
// transport schemes are limited already); the stability of the explicit step where the meridians converge comes from
// the cap cmax on the diffusion numbers, not from an implicit zonal solve; latitude bands are refused by default -- the
// stencil reads two rows beyond the own rows at order 2 and a band's ghost rows cannot be advanced locally.
//
// A latitude band that has opted in (gcm_set_band_hdiff) takes the BAND form of the kernel over its own rows.  The phase
// sits directly behind the corrector, whose exchange has just filled the kGhost = 2 ghost rows a side of u, v, theta
// and q, and the order-2 stencil has radius 2: every own cell sees the single domain's inputs and operations in the
// same order, hence its bits.  j is not periodic there: tile and halo rows j0 - R + r are addressed directly, rows -2,
// -1, H and H + 1 being the ghost rows of the same allocation; only i wraps.  The device tables of a band are
// [8][H + 4], rows -2 .. H + 1, gathered on the host from the tables over the global height at row (row0 + j) mod Hg
// (rank 0's ghost row -1 is global row Hg - 1: the ring wraps as the dynamics do).  The ghost rows themselves cannot
// be diffused (ghost row -1 would need row -3): behind the launch and the copy back they are stale, and the current
// state's edge rows are exchanged once more before anything reads them (gcm_band.hip, band_step_pe_hd; a host-driven
// step: gcm_end_step_diffuse, the caller's exchange, gcm_end_step_begin).  That costs one more message of
// gcm_halo_bytes per neighbour and step.  Deliberately not built: dispatching the edge rows' tiles first, so that the
// exchange hides behind the interior tiles.  The launch is out of place and the interior tiles read the ORIGINAL edge
// rows, so the edge rows cannot be copied back and packed while the interior launch is in flight.
//
// Every operation is rounded on its own: contraction is off for the whole file (the Makefile builds it with
// -ffp-contract=fast-honor-pragmas), host and device, so the host tables are the NumPy restatement's bits and a cell
// gets the same bits whichever tile computes it.
//
// Out of place by construction.  The stencil has radius 2 at order 2: in place, a workgroup would read words another
// has written.  The launch reads the state's fields and writes X' to landing fields of the handle's real type (own rows
// [H][L][W], one per selected field, allocated by the registration or by the first explicit step and kept); no word is
// both read and written by one launch.  The state then takes them over by a device copy on the same stream, NOT by
// exchanging the field pointers: PeBufs::st holds interior-row pointers into allocations with ghost rows, which the
// wide paths of the stage kernels assume 16-byte aligned at fixed offsets, and which the halo segments, the tracers'
// chain, gcm_get_intermediate's stage state and every launch argument built by make_args take by value at queue time
// on three streams; a landing field without ghost rows cannot stand in for them, and one with them would make every
// holder of a pointer follow the exchange.  The copy costs one more read and write of each selected field
// (4 W H L sizeof(T) bytes per field and application in all) and touches nothing else.
//
// The kernel: tile and halo in LDS, see pe25d_hdiff.h for the geometry and its reasoning.  The state's layout is
// [j][k][i]: a tile row of one level is one contiguous run of 128 + 2 order elements.
#pragma clang fp contract(off)
#include "pe25d_host.h"
#include "pe25d_hdiff.h"

#include <cmath>
#include <cstring>

namespace gcm {

static_assert(kHdGhost == kGhost, "a band's ghost rows a side are the diffusion's halo at order 2");

// ---------------------------------------------------------------- the tables and the probe (host)
int hdiff_check(const gcm_hdiff *d, const char *fn, std::string *err) {
    const auto bad = [&](const char *what) { *err = std::string(fn) + ": " + what; return GCM_ERR_ARG; };
    if (!d) return bad("no parameters");
    if (d->order != 1 && d->order != 2) return bad("order must be 1 (del-2) or 2 (del-4)");
    if (d->fields <= 0 || (d->fields & ~(GCM_HDIFF_U | GCM_HDIFF_V | GCM_HDIFF_T | GCM_HDIFF_Q)))
        return bad("fields must be a non-empty mask of GCM_HDIFF_U, _V, _T and _Q");
    if (!std::isfinite(d->nu) || !(d->nu > 0.0)) return bad("nu must be finite and > 0");
    if (!(d->cmax > 0.0 && d->cmax <= 0.125)) return bad("cmax must lie in (0, 1/8]");
    return GCM_OK;
}

int hdiff_tables(int H, const double *dx_j, const double *dx_h, double dy, const gcm_hdiff *d, double dt, double *out, std::string *err) {
    const char *fn = "gcm_hdiff_tables";
    const auto bad = [&](const char *what) { *err = std::string(fn) + ": " + what; return GCM_ERR_ARG; };
    if (H < 1) return bad("H must be 1 or more");
    if (!dx_j || !dx_h || !out) return bad("a null pointer");
    if (int rc = hdiff_check(d, fn, err)) return rc;
    if (!std::isfinite(dt)) return bad("dt must be finite");
    const double nudt = d->nu * dt;
    const double s = d->order == 1 ? nudt : std::sqrt(nudt);
    const double cmax = d->cmax;
    const double dy2 = dy * dy;
    const double ay = std::fmin(s / dy2, cmax);
    double *ax = out, *bn = ax + H, *bs = bn + H, *area = bs + H, *axv = area + H, *bnv = axv + H, *bsv = bnv + H, *areav = bsv + H;
    for (int j = 0; j < H; ++j) {
        const int jn = j == 0 ? H - 1 : j - 1, js = j == H - 1 ? 0 : j + 1;
        const double xj = dx_j[j], xh = dx_h[j], xhn = dx_h[jn], xjs = dx_j[js];
        const double xj2 = xj * xj;
        ax[j] = std::fmin(s / xj2, cmax);
        const double hsum = xhn + xh;
        const double a = hsum * dy;
        area[j] = a * 0.5;
        const double ws = xh * dy;
        const double wn = xhn * dy;
        const double ns = ay * ws;
        const double nn = ay * wn;
        bs[j] = ns / area[j];
        bn[j] = nn / area[j];
        const double xh2 = xh * xh;
        axv[j] = std::fmin(s / xh2, cmax);
        const double jsum = xj + xjs;
        const double av = jsum * dy;
        areav[j] = av * 0.5;
        const double wsv = xjs * dy;
        const double wnv = xj * dy;
        const double nsv = ay * wsv;
        const double nnv = ay * wnv;
        bsv[j] = nsv / areav[j];
        bnv[j] = nnv / areav[j];
    }
    return GCM_OK;
}

// D of one level [H][W] with the rows' coefficients, periodic both ways
static void hdiff_level(int H, int W, const double *ax, const double *bn, const double *bs, const double *X, double *D) {
    for (int j = 0; j < H; ++j) {
        const double *c = X + (size_t)j * W, *n = X + (size_t)(j == 0 ? H - 1 : j - 1) * W, *s = X + (size_t)(j == H - 1 ? 0 : j + 1) * W;
        for (int i = 0; i < W; ++i) {
            const int iw = i == 0 ? W - 1 : i - 1, ie = i == W - 1 ? 0 : i + 1;
            D[(size_t)j * W + i] = hdiff_cell(c[i], c[iw], c[ie], n[i], s[i], ax[j], bn[j], bs[j]);
        }
    }
}

int hdiff_apply(int H, int W, int nlev, const double *tab4, int order, const double *X, double *out, std::string *err) {
    const char *fn = "gcm_hdiff_apply";
    const auto bad = [&](const char *what) { *err = std::string(fn) + ": " + what; return GCM_ERR_ARG; };
    if (H < 1 || W < 1 || nlev < 1) return bad("H, W and nlev must be 1 or more");
    if (!tab4 || !X || !out) return bad("a null pointer");
    if (order != 1 && order != 2) return bad("order must be 1 or 2");
    const double *ax = tab4, *bn = ax + H, *bs = bn + H;
    const size_t n = (size_t)H * W;
    std::vector<double> Y(n), D(order == 2 ? n : 0);
    for (int k = 0; k < nlev; ++k) {
        const double *x = X + k * n;
        double *o = out + k * n;
        hdiff_level(H, W, ax, bn, bs, x, Y.data());
        if (order == 1) {
            for (size_t c = 0; c < n; ++c) o[c] = x[c] + Y[c];
        } else {
            hdiff_level(H, W, ax, bn, bs, Y.data(), D.data());
            for (size_t c = 0; c < n; ++c) o[c] = x[c] - D[c];
        }
    }
    return GCM_OK;
}

// D of rows [r0, r1) of one band level [Hb + 4][W] (row r is band row r - 2) with the rows' coefficients, periodic in i
// only: rows r - 1 and r + 1 are addressed directly
static void hdiff_band_level(int r0, int r1, int W, const double *ax, const double *bn, const double *bs, const double *X, double *D) {
    for (int r = r0; r < r1; ++r) {
        const double *c = X + (size_t)r * W, *n = c - W, *s = c + W;
        for (int i = 0; i < W; ++i) {
            const int iw = i == 0 ? W - 1 : i - 1, ie = i == W - 1 ? 0 : i + 1;
            D[(size_t)r * W + i] = hdiff_cell(c[i], c[iw], c[ie], n[i], s[i], ax[r], bn[r], bs[r]);
        }
    }
}

// gcm_hdiff_apply_band: the host build of the band walk.  Order 2 forms Y on rows -1 .. Hb from rows -2 .. Hb + 1
int hdiff_apply_band(int Hb, int W, int nlev, const double *tab4, int order, const double *X, double *out, std::string *err) {
    const char *fn = "gcm_hdiff_apply_band";
    const auto bad = [&](const char *what) { *err = std::string(fn) + ": " + what; return GCM_ERR_ARG; };
    if (Hb < 1 || W < 1 || nlev < 1) return bad("Hb, W and nlev must be 1 or more");
    if (!tab4 || !X || !out) return bad("a null pointer");
    if (order != 1 && order != 2) return bad("order must be 1 or 2");
    const int HT = Hb + 4;
    const double *ax = tab4, *bn = ax + HT, *bs = bn + HT;
    const size_t n = (size_t)HT * W, own = (size_t)Hb * W;
    std::vector<double> Y(n, 0.0), D(order == 2 ? n : 0, 0.0);
    for (int k = 0; k < nlev; ++k) {
        const double *x = X + k * n;
        double *o = out + k * own;
        if (order == 1) {
            hdiff_band_level(2, Hb + 2, W, ax, bn, bs, x, Y.data());
            for (size_t c = 0; c < own; ++c) o[c] = x[2 * (size_t)W + c] + Y[2 * (size_t)W + c];
        } else {
            hdiff_band_level(1, Hb + 3, W, ax, bn, bs, x, Y.data());
            hdiff_band_level(2, Hb + 2, W, ax, bn, bs, Y.data(), D.data());
            for (size_t c = 0; c < own; ++c) o[c] = x[2 * (size_t)W + c] - D[2 * (size_t)W + c];
        }
    }
    return GCM_OK;
}

// the tables of a band, [8][Hb + 4]: row r of each is row (row0 - 2 + r) mod Hg of the table over the global height
void hdiff_band_tables(int Hg, int row0, int Hb, const double *glob, double *out) {
    const int HT = Hb + 4;
    for (int t = 0; t < 8; ++t)
        for (int r = 0; r < HT; ++r) {
            int j = (row0 - 2 + r) % Hg;
            if (j < 0) j += Hg;
            out[(size_t)t * HT + r] = glob[(size_t)t * Hg + j];
        }
}

// ---------------------------------------------------------------- the kernel
template <typename T>
struct HdArgsT {
    const T *src[GCM_NFIELDS - 1];   // the selected fields of the state, [j][k][i], interior row 0
    T *dst[GCM_NFIELDS - 1];         // their landing fields, [j][k][i], own rows only
    int isv[GCM_NFIELDS - 1];        // 1: the field lies on v rows (the second four tables)
    const double *tab;               // [8][H]; a band: [8][H + 4], rows -2 .. H + 1
    int W, H, L;
};

__device__ inline int hd_wrap(int x, int n) { return x < 0 ? x + n : x >= n ? x - n : x; }
// a row index: periodic on a single domain, as it is on a band (rows -2 .. H + 1 exist there)
template <bool BAND>
__device__ inline int hd_row(int j, int H) { return BAND ? j : hd_wrap(j, H); }

// grid (strips of kHdCols columns, tiles of kHdRows rows, selected field x level).  W >= 4 and H >= 4: an index a halo
// of two cells reaches wraps once at the most.  The work of a phase is laid out so that a row is wave-uniform and a
// lane owns a column: row addresses and the rows' coefficients are scalar (the table is read through the scalar
// cache, no LDS copy), no index is divided, and a thread that marches down its column keeps the two values above the
// new row in registers -- three LDS reads a cell instead of five.
// BAND: a latitude band's own rows [0, H).  j is not periodic: a row index is used as it is (rows -2, -1, H, H + 1 are
// the ghost rows of the same allocation, and the table has their coefficients); H >= 2.  Everything else is the same code
template <typename T, int ORDER, bool BAND = false>
__global__ __launch_bounds__(kHdThreads) void pe_hdiff_kernel(HdArgsT<T> a) {
    constexpr int R = ORDER;
    constexpr int XW = kHdCols + 2 * R, XR = kHdRows + 2 * R;
    constexpr int YW = kHdCols + 2, YR = kHdRows + 2;
    static_assert(kHdThreads == 256 && kHdCols == 128 && kHdRows % 2 == 0, "two half workgroups of 128 lanes, one lane a column");
    __shared__ double xs[XR * XW];
    __shared__ double ys[ORDER == 2 ? YR * YW : 1];
    const int W = a.W, H = a.H, L = a.L;
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // 0 .. 3
    const int half = wave >> 1;                                    // which half of the rows a thread marches
    const int col = tid & (kHdCols - 1);                           // ... in this column of the tile
    const int i0 = (int)blockIdx.x * kHdCols, j0 = (int)blockIdx.y * kHdRows;
    const int f = (int)blockIdx.z / L, k = (int)blockIdx.z - f * L;
    // (selected one by one: an index into the by-value arrays would put them into scratch)
    const T *src = f == 0 ? a.src[0] : f == 1 ? a.src[1] : f == 2 ? a.src[2] : a.src[3];
    T *dst = f == 0 ? a.dst[0] : f == 1 ? a.dst[1] : f == 2 ? a.dst[2] : a.dst[3];
    const int isv = f == 0 ? a.isv[0] : f == 1 ? a.isv[1] : f == 2 ? a.isv[2] : a.isv[3];
    const int TH = BAND ? H + 2 * kHdGhost : H;                     // rows of a table; a band's row j is entry j + 2
    const double *ax_t = a.tab + (long)(isv ? 4 : 0) * TH + (BAND ? kHdGhost : 0), *bn_t = ax_t + TH, *bs_t = bn_t + TH;
    const int nr = min(kHdRows, H - j0), nc = min(kHdCols, W - i0);   // the tile's own cells (a partial last tile)
    const int lr = nr + 2 * R, lc = nc + 2 * R;
    const long rs = (long)L * W;                                   // elements from a row to the next
    const T *lev = src + (long)k * W;                              // level k of row 0
    // the coefficients of the rows a thread marches, rows j0 - 1 + 8 half + m, read ahead of everything else: behind the
    // first store the compiler may no longer take the table through the scalar cache.  Y row r = 9 half + n is m = n + half,
    // row r = 8 half + n of the tile is m = n + 1.  (A row beyond the tile's last Y row is never used: clamped into the table)
    constexpr int kCoef = kHdRows / 2 + 2;
    double cax[kCoef], cbn[kCoef], cbs[kCoef];
#pragma unroll
    for (int m = 0; m < kCoef; ++m) {
        const int j = hd_row<BAND>(min(j0 - 1 + (kHdRows / 2) * half + m, j0 + nr), H);
        cax[m] = ax_t[j];
        cbn[m] = bn_t[j];
        cbs[m] = bs_t[j];
    }

    // ---- tile and halo.  Wave w takes rows w, w + 4, ...: columns lane and lane + 64 of each, then the 2 R columns
    // beyond 128 of every row, one element a thread.  Every request is issued before the first value is used
    constexpr int kRowIt = (XR + 3) / 4, kTail = 2 * R * XR;
    const int ia = hd_wrap(i0 - R + lane, W), ib = hd_wrap(i0 - R + lane + 64, W);
    T va[kRowIt], vb[kRowIt], vt = (T)0;
#pragma unroll
    for (int n = 0; n < kRowIt; ++n) {
        const int r = wave + 4 * n;
        va[n] = vb[n] = (T)0;
        if (r < lr) {
            const T *row = lev + (long)hd_row<BAND>(j0 - R + r, H) * rs;
            if (lane < lc) va[n] = row[ia];
            if (lane + 64 < lc) vb[n] = row[ib];
        }
    }
    const int tr = tid / (2 * R), tc = 2 * 64 + tid % (2 * R);
    if (tid < kTail && tr < lr && tc < lc) vt = lev[(long)hd_row<BAND>(j0 - R + tr, H) * rs + hd_wrap(i0 - R + tc, W)];
#pragma unroll
    for (int n = 0; n < kRowIt; ++n) {
        const int r = wave + 4 * n;
        if (r < XR) {
            xs[r * XW + lane] = (double)va[n];
            xs[r * XW + lane + 64] = (double)vb[n];
        }
    }
    if (tid < kTail) xs[tr * XW + tc] = (double)vt;
    __syncthreads();

    if (ORDER == 2) {
        // ---- Y on the tile and one cell a side: Y row r is row j0 - 1 + r, which is X row r + 1.  A thread marches
        // half of the YR rows down column `col`; the two columns beyond 128 take one cell a thread
        constexpr int kRows = YR / 2;
        static_assert(kRows == kHdRows / 2 + 1, "the coefficient rows above");
        const int r0 = half * kRows;
        if (col < nc + 2) {
            const double *x = xs + (r0 + 1) * XW + (col + 1);
            double xn = x[-XW], xc = x[0];
#pragma unroll
            for (int n = 0; n < kRows; ++n) {
                const int r = r0 + n;
                if (r >= nr + 2) break;
                const double xso = x[XW];
                ys[r * YW + col] = hdiff_cell(xc, x[-1], x[1], xn, xso, half ? cax[n + 1] : cax[n], half ? cbn[n + 1] : cbn[n],
                                              half ? cbs[n + 1] : cbs[n]);
                xn = xc;
                xc = xso;
                x += XW;
            }
        }
        const int r = tid >> 1, c = kHdCols + (tid & 1);
        if (tid < 2 * YR && r < nr + 2 && c < nc + 2) {
            const int j = hd_row<BAND>(j0 - 1 + r, H);
            const double *x = xs + (r + 1) * XW + (c + 1);
            ys[r * YW + c] = hdiff_cell(x[0], x[-1], x[1], x[-XW], x[XW], ax_t[j], bn_t[j], bs_t[j]);
        }
        __syncthreads();
    }

    // ---- X' on the tile: a thread marches half of the rows down column `col`
    if (col >= nc) return;
    constexpr int kRows = kHdRows / 2;
    const int r0 = half * kRows;
    const double *z = ORDER == 2 ? ys + (r0 + 1) * YW + (col + 1) : xs + (r0 + 1) * XW + (col + 1);
    constexpr int ZW = ORDER == 2 ? YW : XW;
    double zn = z[-ZW], zc = z[0];
    T *out = dst + ((long)(j0 + r0) * L + k) * W + (i0 + col);
#pragma unroll
    for (int n = 0; n < kRows; ++n) {
        const int r = r0 + n;
        if (r >= nr) break;
        const double zs = z[ZW];
        const double d = hdiff_cell(zc, z[-1], z[1], zn, zs, cax[n + 1], cbn[n + 1], cbs[n + 1]);
        double res;
        if (ORDER == 2) res = xs[(r + 2) * XW + (col + 2)] - d;
        else res = zc + d;
        *out = (T)res;
        zn = zc;
        zc = zs;
        z += ZW;
        out += rs;
    }
}

// ---------------------------------------------------------------- the registration, the tables' way to the device
static const int kHdField[GCM_NFIELDS - 1] = {GCM_U, GCM_V, GCM_T, GCM_Q};
static const int kHdBit[GCM_NFIELDS - 1] = {GCM_HDIFF_U, GCM_HDIFF_V, GCM_HDIFF_T, GCM_HDIFF_Q};

int pe25d_hdiff_fits(const Pe25d *m, const char *fn, std::string *err) {
    const auto no = [&](const char *what) { *err = std::string(fn) + ": " + what; return GCM_ERR_UNSUPPORTED; };
    if (!m->wrap && !m->hdiff.band)
        return no("single domains only (the stencil reads two rows beyond a latitude band's own rows, and its ghost rows cannot be advanced locally: gcm_set_band_hdiff)");
    if (!m->wrap) {
        // (an opted-in band: rows are addressed directly, so only i must wrap once at the most; kGhost own rows at the least,
        // as the exchange needs anyway)
        if (m->W < 4 || m->H < kGhost || m->Hg < 4) return no("a band needs W >= 4, 2 own rows or more and a global height of 4 or more");
        return GCM_OK;
    }
    if (m->W < 4 || m->H < 4) return no("W and H must be 4 or more (the halo of two cells wraps once only)");
    return GCM_OK;
}

// gcm_set_band_hdiff: a band takes the phase over its own rows and one more exchange per step behind it
int pe25d_set_band_hdiff(Pe25d *m, bool on, std::string *err) {
    if (m->wrap) {
        if (!on) return GCM_OK;
        *err = "gcm_set_band_hdiff: GCM_PE25D latitude bands only (a single domain takes gcm_set_hdiff directly)";
        return GCM_ERR_UNSUPPORTED;
    }
    if (!on && m->hdiff.on) {
        *err = "gcm_set_band_hdiff: the horizontal diffusion is registered (gcm_set_hdiff(NULL) first)";
        return GCM_ERR_STATE;
    }
    m->hdiff.band = on;
    return GCM_OK;
}
bool pe25d_band_hdiff(const Pe25d *m) { return !m->wrap && m->hdiff.band; }
// a band's own rows diffused for the step gcm_end_step_begin ends (gcm_end_step_diffuse sets it, begin takes it)
bool pe25d_band_hdiff_done(const Pe25d *m) { return m->hdiff.band_done; }
void pe25d_set_band_hdiff_done(Pe25d *m, bool done) { m->hdiff.band_done = done; }

static void hdiff_free(Pe25d *m, void *p) {
    m->allocs.erase(std::remove(m->allocs.begin(), m->allocs.end(), p), m->allocs.end());
    (void)hipFree(p);
}

// the landing fields of `fields` in place: allocated here where they are not yet.  A failure frees what this call allocated
static int hdiff_landing(Pe25d *m, int fields, std::string *err) {
    PeHdiff &z = m->hdiff;
    const size_t bytes = elem_size(m) * (size_t)m->H * m->L * m->W;
    void *made[GCM_NFIELDS - 1] = {};
    for (int n = 0; n < GCM_NFIELDS - 1; ++n) {
        if (!(fields & kHdBit[n]) || z.land[kHdField[n]]) continue;
        char *d = nullptr;
        if (!dev_upload<char>(m, &d, nullptr, bytes)) {
            for (int e = 0; e < n; ++e)
                if (made[e]) { hdiff_free(m, made[e]); z.land[kHdField[e]] = nullptr; }
            *err = "hip: horizontal diffusion: landing field allocation failed";
            return GCM_ERR_HIP;
        }
        made[n] = z.land[kHdField[n]] = d;
    }
    return GCM_OK;
}

int pe25d_set_hdiff(Pe25d *m, const gcm_hdiff *d, hipStream_t s, std::string *err) {
    PeHdiff &z = m->hdiff;
    if (!d) {
        bool any = z.tab != nullptr;
        for (void *p : z.land) any = any || p;
        if (any)                                             // (a launch or a copy may still use them)
            if (int rc = hip_rc(hipStreamSynchronize(s), "gcm_set_hdiff", err)) return rc;
        for (void *&p : z.land)
            if (p) { hdiff_free(m, p); p = nullptr; }
        if (z.tab) { hdiff_free(m, z.tab); z.tab = nullptr; }
        z.key.clear();
        z.on = false;
        z.band_done = false;
        return GCM_OK;
    }
    if (int rc = hdiff_check(d, "gcm_set_hdiff", err)) return rc;
    if (int rc = pe25d_hdiff_fits(m, "gcm_set_hdiff", err)) return rc;
    if (int rc = hdiff_landing(m, d->fields, err)) return rc;
    z.par = *d;
    z.on = true;
    return GCM_OK;
}

bool pe25d_hdiff_on(const Pe25d *m) { return m->hdiff.on; }
const gcm_hdiff *pe25d_hdiff_par(const Pe25d *m) { return m->hdiff.on ? &m->hdiff.par : nullptr; }

int pe25d_hdiff_tables(Pe25d *m, const gcm_hdiff *d, double dt, hipStream_t s, std::string *err) {
    if (int rc = hdiff_check(d, "horizontal diffusion", err)) return rc;
    if (!std::isfinite(dt)) { *err = "horizontal diffusion: dt must be finite"; return GCM_ERR_ARG; }
    if (int rc = pe25d_hdiff_fits(m, "horizontal diffusion", err)) return rc;
    if (int rc = hdiff_landing(m, d->fields, err)) return rc;
    PeHdiff &z = m->hdiff;
    const int Hg = m->wrap ? m->H : m->Hg;                 // (the tables span the global height; a band gathers its rows)
    z.fields = d->fields;                                  // (the mask is not part of the tables)
    std::vector<double> key = {(double)d->order, d->nu, d->cmax, dt};
    if (z.tab && z.key.size() == key.size() && !memcmp(z.key.data(), key.data(), sizeof(double) * key.size())) return GCM_OK;
    std::vector<double> T((size_t)8 * Hg);
    if (int rc = hdiff_tables(Hg, m->dxj_host.data(), m->dxh_host.data(), m->cfg.dy, d, dt, T.data(), err)) return rc;
    if (!m->wrap) {
        std::vector<double> B((size_t)8 * (m->H + 2 * kGhost));
        hdiff_band_tables(Hg, m->cfg.row0, m->H, T.data(), B.data());
        T.swap(B);
    }
    // A change is rare (another dt, another registration): everything queued so far may still read the tables in place,
    // so it ends first, and the upload is synchronous (as pe25d_hs_tables)
    if (hipStreamSynchronize(s) != hipSuccess) { *err = "hip: horizontal diffusion: the launches ahead of the table upload failed"; return GCM_ERR_HIP; }
    if (!z.tab && !dev_upload<double>(m, &z.tab, nullptr, T.size())) { *err = "hip: horizontal diffusion table allocation failed"; return GCM_ERR_HIP; }
    if (hipMemcpy(z.tab, T.data(), sizeof(double) * T.size(), hipMemcpyHostToDevice) != hipSuccess) {
        z.key.clear();
        *err = "hip: horizontal diffusion table upload failed"; return GCM_ERR_HIP;
    }
    z.key.swap(key);
    z.order = d->order;
    return GCM_OK;
}

// ---------------------------------------------------------------- the launch
template <typename T>
static int hd_launch(Pe25d *m, int set, hipStream_t s, std::string *err) {
    PeBufs<T> &B = bufs<T>(m);
    const PeHdiff &z = m->hdiff;
    HdArgsT<T> a{};
    int nf = 0;
    for (int n = 0; n < GCM_NFIELDS - 1; ++n) {
        if (!(z.fields & kHdBit[n])) continue;
        a.src[nf] = B.st[set][kHdField[n]];
        a.dst[nf] = (T *)z.land[kHdField[n]];
        a.isv[nf] = kHdField[n] == GCM_V ? 1 : 0;
        ++nf;
    }
    a.tab = z.tab;
    a.W = m->W; a.H = m->H; a.L = m->L;
    const HdiffGrid g = hdiff_grid(m->W, m->H, m->L, nf);
    const dim3 grid(g.tiles_i, g.tiles_j, g.z);
    if (!m->wrap) {                                        // a band that has opted in: its own rows, rows not periodic
        if (z.order == 2) hipLaunchKernelGGL((pe_hdiff_kernel<T, 2, true>), grid, dim3(kHdThreads), 0, s, a);
        else hipLaunchKernelGGL((pe_hdiff_kernel<T, 1, true>), grid, dim3(kHdThreads), 0, s, a);
    } else if (z.order == 2) hipLaunchKernelGGL((pe_hdiff_kernel<T, 2>), grid, dim3(kHdThreads), 0, s, a);
    else hipLaunchKernelGGL((pe_hdiff_kernel<T, 1>), grid, dim3(kHdThreads), 0, s, a);
    if (hipGetLastError() != hipSuccess) { *err = "hip: horizontal diffusion kernel launch failed"; return GCM_ERR_HIP; }
    // the state takes the landing fields over: the own rows of a field are one contiguous run
    const size_t bytes = sizeof(T) * (size_t)m->H * m->L * m->W;
    for (int n = 0; n < nf; ++n)
        if (int rc = hip_rc(hipMemcpyAsync(const_cast<T *>(a.src[n]), a.dst[n], bytes, hipMemcpyDeviceToDevice, s), "horizontal diffusion", err)) return rc;
    return GCM_OK;
}

int pe25d_hdiff_rows(Pe25d *m, int set, bool keep_ghosts, hipStream_t s, std::string *err) {
    const PeHdiff &z = m->hdiff;
    if (!z.tab || z.key.empty() || !z.fields) { *err = "horizontal diffusion: no tables in place"; return GCM_ERR_STATE; }
    for (int n = 0; n < GCM_NFIELDS - 1; ++n)
        if ((z.fields & kHdBit[n]) && !z.land[kHdField[n]]) { *err = "horizontal diffusion: no landing fields in place"; return GCM_ERR_STATE; }
    if (int rc = pe25d_hdiff_fits(m, "horizontal diffusion", err)) return rc;
    if (set < 0) set = m->cur_i;
    // the launch and the copies write u and v (and theta, q): as pe25d_hs_rows, the fork at the last K4 is invalidated and
    // the state's column sums are stale.  A mask without u and v goes the same way: one path, and theta is written as well
    pe25d_phase_wrote(m, set, keep_ghosts, true);
    return m->f32 ? hd_launch<float>(m, set, s, err) : hd_launch<double>(m, set, s, err);
}

// gcm_hdiff_plan: at the registered order, else at order 2
int pe25d_hdiff_plan(const Pe25d *m, int *out, int nout) {
    if (!out || nout < GCM_HDIFF_PLAN_WORDS) return GCM_ERR_ARG;
    const PeHdiff &z = m->hdiff;
    const int order = z.on ? z.par.order : 2;
    int nf = 0;
    const int fields = z.on ? z.par.fields : (GCM_HDIFF_U | GCM_HDIFF_V | GCM_HDIFF_T);
    for (int n = 0; n < GCM_NFIELDS - 1; ++n) nf += (fields & kHdBit[n]) ? 1 : 0;
    const HdiffGrid g = hdiff_grid(m->W, m->H, m->L, nf);
    out[0] = kHdRows; out[1] = kHdCols; out[2] = g.tiles_i; out[3] = g.tiles_j; out[4] = g.z;
    out[5] = (int)hdiff_lds_bytes(order); out[6] = 1;
    return GCM_OK;
}

}  // namespace gcm

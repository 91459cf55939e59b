// GCM_PE25D, slab mixed-layer ocean with a recorded surface and top-of-atmosphere budget (gcm_set_slab_ocean,
// gcm_slab_ocean_apply): the ground temperature becomes the temperature of a slab of heat capacity C that is heated by
// the net radiation at the surface and pays for the sensible heat and the evaporation the boundary layer takes from it,
// directly behind the boundary layer and ahead of the convective adjustment.  The contract: include/gcmcore.h.
//
// The phase owns no physics of the atmosphere.  It reads GCM_SLAB_WORDS float64 flux words per cell, which the phases
// that know them store while the slab is registered and at no other time:
//   SC, SW_SFC, LW_DOWN, LW_UP, OLR   W / m^2   pe_radiation_kernel, its BUDGET instantiations (pe25d_physics.hip), which
//                                              leave the ground temperature alone
//   SH_J   J / m^2,  EVAP_KG   kg / m^2        pe_bl_theta_q_kernel (pe25d_boundary_layer.hip): the step's own increments
//                                              of shf and evap
// and advances the cell (slab_cell, pe25d_slab_ocean.h):
//   R = (S + B) - U_s;  E1 = dt R;  E2 = E1 - SH_J;  E3 = E2 - Lv EVAP_KG;  E4 = E3 + dt Q;  gt' = gt + E4 / C
// The words of a phase that is not registered are taken as zero, and stored as zero (`mask`).  The same launch adds the
// cell's terms to GCM_SLAB_SUMS float64 sums (slab_sums), own rows only.
//
// Every operation is float64 and rounded on its own: contraction is off for the whole file (the Makefile builds it with
// -ffp-contract=fast-honor-pragmas), host and device, and the host probe gcm_slab_ocean_cells evaluates the very routine
// the kernel calls.
//
// pe_slab_ocean_kernel: one lane per cell, a workgroup is one wave of 64 consecutive columns of one row, grid (tiles of
// 64 columns, rows), the last tile ragged.  A lane reads and writes the words of its own cell only: one writer per word,
// no atomics, no LDS, no scratch.
#pragma clang fp contract(off)
#include "pe25d_host.h"
#include "pe25d_slab_ocean.h"

namespace gcm {

constexpr int kSlabLanes = 64;
enum { kSlabMaskRadiation = 1, kSlabMaskBoundary = 2 };

struct SlabArgs {
    double *gt;                      // [j][i], interior row 0
    double *words;                   // GCM_SLAB_WORDS fields [j][i] of `wstride` words each, interior row 0
    double *sums;                    // GCM_SLAB_SUMS fields [H][W], or null: the launch accumulates nothing
    const double *cap, *qflux;       // [H][W], or null: the scalar C; 0
    long wstride, sstride;
    double C, Lv, dt;
    int mask;                        // kSlabMask*: the words that are meaningful; the others are read as 0 and stored as 0
    int W, H;
    int j0, n0, jb0;                 // rows of the launch: [j0, j0 + n0), then from jb0 on (a band's ghost rows)
};

__global__ __launch_bounds__(kSlabLanes) void pe_slab_ocean_kernel(SlabArgs a) {
    const int i = (int)blockIdx.x * kSlabLanes + (int)threadIdx.x;
    const int j = (int)blockIdx.y < a.n0 ? a.j0 + (int)blockIdx.y : a.jb0 + ((int)blockIdx.y - a.n0);
    if (i >= a.W) return;
    const long c2 = (long)j * a.W + i;
    const bool own = j >= 0 && j < a.H;
    double *const w = a.words + c2;
    SlabWords f{};
    if (a.mask & kSlabMaskRadiation) {
        f.sc = w[0]; f.sw_sfc = w[a.wstride]; f.lw_down = w[2 * a.wstride]; f.lw_up = w[3 * a.wstride]; f.olr = w[4 * a.wstride];
    } else {
        w[0] = 0.0; w[a.wstride] = 0.0; w[2 * a.wstride] = 0.0; w[3 * a.wstride] = 0.0; w[4 * a.wstride] = 0.0;
    }
    if (a.mask & kSlabMaskBoundary) {
        f.sh_j = w[5 * a.wstride]; f.evap_kg = w[6 * a.wstride];
    } else {
        w[5 * a.wstride] = 0.0; w[6 * a.wstride] = 0.0;
    }
    // (the registered fields hold own rows only: the host keeps a launch with either to the own rows)
    const double C = a.cap ? a.cap[c2] : a.C;
    const double Q = a.qflux ? a.qflux[c2] : 0.0;
    const SlabCell c = slab_cell(a.gt[c2], C, a.dt, a.Lv, f, Q);
    a.gt[c2] = c.gt;
    if (a.sums && own) {
        double add[GCM_SLAB_SUMS];
        slab_sums(add, a.dt, a.Lv, f, Q, c.gt);
#pragma unroll
        for (int n = 0; n < GCM_SLAB_SUMS; ++n) a.sums[n * a.sstride + c2] = a.sums[n * a.sstride + c2] + add[n];
    }
}

// ---------------------------------------------------------------- parameters and the host probe
static bool slab_capacity_ok(double c) { return c > 0.0; }     // (NaN fails the comparison; +inf holds the cell)

int slab_ocean_check(const gcm_slab_ocean *so, const char *fn, std::string *err) {
    const auto bad = [&](const char *what) { *err = std::string(fn) + ": " + what; return GCM_ERR_ARG; };
    if (!so) return bad("no parameters");
    if (!slab_capacity_ok(so->heat_capacity)) return bad("heat_capacity must be > 0 (+inf holds the temperature)");
    if (!(so->Lv > 0.0) || !std::isfinite(so->Lv)) return bad("Lv must be finite and > 0");
    return GCM_OK;
}

// a capacity field: every cell > 0, +inf allowed; a heat-flux field: finite
static int slab_fields_check(size_t n, const double *cap, const double *qflux, const char *fn, std::string *err) {
    for (size_t c = 0; cap && c < n; ++c)
        if (!slab_capacity_ok(cap[c])) { *err = std::string(fn) + ": every cell of the capacity field must be > 0 (+inf holds the temperature)"; return GCM_ERR_ARG; }
    for (size_t c = 0; qflux && c < n; ++c)
        if (!std::isfinite(qflux[c])) { *err = std::string(fn) + ": the heat-flux field must be finite"; return GCM_ERR_ARG; }
    return GCM_OK;
}

int slab_ocean_cells(int n, const gcm_slab_ocean *so, double dt, const double *gt, const double *C, const double *words,
                     const double *Q, double *gt_out, double *E4_out, std::string *err) {
    const char *fn = "gcm_slab_ocean_cells";
    if (int rc = slab_ocean_check(so, fn, err)) return rc;
    if (n < 0 || !std::isfinite(dt) || (n > 0 && (!gt || !words || !gt_out))) {
        *err = std::string(fn) + ": n must be >= 0, dt finite, gt, words and gt_out are required";
        return GCM_ERR_ARG;
    }
    if (int rc = slab_fields_check((size_t)n, C, Q, fn, err)) return rc;
    for (int i = 0; i < n; ++i) {
        const double *w = words + i;
        const SlabWords f{w[0], w[(size_t)n], w[(size_t)2 * n], w[(size_t)3 * n], w[(size_t)4 * n], w[(size_t)5 * n], w[(size_t)6 * n]};
        const SlabCell c = slab_cell(gt[i], C ? C[i] : so->heat_capacity, dt, so->Lv, f, Q ? Q[i] : 0.0);
        gt_out[i] = c.gt;
        if (E4_out) E4_out[i] = c.E4;
    }
    return GCM_OK;
}

// ---------------------------------------------------------------- the handle's side
static size_t slab_cells(const Pe25d *m) { return (size_t)m->H * m->W; }
static size_t slab_word_stride(const Pe25d *m) { return rows_alloc(m) * m->W; }

static void slab_free(Pe25d *m, double **p) {
    if (!*p) return;
    m->allocs.erase(std::remove(m->allocs.begin(), m->allocs.end(), (void *)*p), m->allocs.end());
    (void)hipFree(*p);
    *p = nullptr;
}

// every stream a slab launch or a launch that stores flux words may still run on
static int slab_quiet(Pe25d *m, const char *fn, hipStream_t s, std::string *err) {
    if (int rc = hip_rc(hipStreamSynchronize(s), fn, err)) return rc;
    if (m->aux) return hip_rc(hipStreamSynchronize(m->aux), fn, err);
    return GCM_OK;
}

// the flux words in place (zero when they are allocated)
static int slab_words_alloc(Pe25d *m, const char *fn, std::string *err) {
    if (m->slab.words) return GCM_OK;
    if (!dev_upload<double>(m, &m->slab.words, nullptr, (size_t)GCM_SLAB_WORDS * slab_word_stride(m))) {
        *err = std::string("hip: ") + fn + " allocation failed"; return GCM_ERR_HIP;
    }
    return GCM_OK;
}

bool pe25d_slab_ocean_on(const Pe25d *m) { return m->slab.on; }

// word `n` of the flux words at interior row 0; null without a registration (what the radiation and the boundary layer ask)
double *pe25d_slab_ocean_word(const Pe25d *m, int n) {
    return m->slab.on ? m->slab.words + (size_t)n * slab_word_stride(m) + (size_t)kGhost * m->W : nullptr;
}

int pe25d_set_slab_ocean(Pe25d *m, const gcm_slab_ocean *so, const double *cap, const double *qflux, hipStream_t s, std::string *err) {
    const char *fn = "gcm_set_slab_ocean";
    PeSlab &z = m->slab;
    if (!so) {
        if (!z.words && !z.sums) return GCM_OK;
        if (int rc = slab_quiet(m, fn, s, err)) return rc;
        slab_free(m, &z.words); slab_free(m, &z.sums); slab_free(m, &z.cap); slab_free(m, &z.qflux);
        z = PeSlab{};
        return GCM_OK;
    }
    if (int rc = slab_ocean_check(so, fn, err)) return rc;
    if (int rc = slab_fields_check(slab_cells(m), cap, qflux, fn, err)) return rc;
    if (!m->gt_set) { *err = std::string(fn) + ": set the ground temperature first (gcm_set_ground)"; return GCM_ERR_STATE; }
    if (int rc = slab_quiet(m, fn, s, err)) return rc;
    // what is new is built aside: an allocation that fails leaves the registration in place as it was
    double *sums = nullptr, *ncap = nullptr, *nq = nullptr;
    bool ok = z.sums || dev_upload<double>(m, &sums, nullptr, (size_t)GCM_SLAB_SUMS * slab_cells(m));
    ok = ok && (!cap || dev_upload<double>(m, &ncap, cap, slab_cells(m)));
    ok = ok && (!qflux || dev_upload<double>(m, &nq, qflux, slab_cells(m)));
    ok = ok && slab_words_alloc(m, fn, err) == GCM_OK;
    if (!ok) {
        slab_free(m, &sums); slab_free(m, &ncap); slab_free(m, &nq);
        *err = std::string("hip: ") + fn + " allocation failed";
        return GCM_ERR_HIP;
    }
    if (z.sums) {
        if (int rc = hip_rc(hipMemset(z.sums, 0, sizeof(double) * GCM_SLAB_SUMS * slab_cells(m)), fn, err)) {
            slab_free(m, &ncap); slab_free(m, &nq);
            return rc;
        }
    } else {
        z.sums = sums;
    }
    slab_free(m, &z.cap); slab_free(m, &z.qflux);
    z.cap = ncap; z.qflux = nq;
    z.par = *so;
    z.seconds = 0.0; z.n = 0;
    z.on = true;
    return GCM_OK;
}

// rows [j0, j1) and [jb0, jb1) (a band's ghost rows: negative, or >= H) on `s` with the parameters `so`; mask: the words
// that are meaningful; accumulate: the own rows' terms go to the registered sums and the call counts as one application
static int slab_launch(Pe25d *m, const gcm_slab_ocean &so, int j0, int j1, int jb0, int jb1, double dt, int mask, bool accumulate,
                       hipStream_t s, std::string *err) {
    PeSlab &z = m->slab;
    if (z.cap || z.qflux) {                                // the fields hold own rows: the ghost rows' temperature comes with the next message
        j0 = std::max(j0, 0); j1 = std::min(j1, m->H);
        jb0 = jb1 = 0;
    }
    if (j0 < -kGhost || j1 > m->H + kGhost || (jb1 > jb0 && (jb0 < -kGhost || jb1 > m->H + kGhost))) {
        *err = "slab ocean: rows outside the handle's allocation"; return GCM_ERR_ARG;
    }
    const int n0 = std::max(0, j1 - j0), nrows = n0 + std::max(0, jb1 - jb0);
    if (nrows > 0) {
        SlabArgs a{};
        a.gt = m->gt;
        a.wstride = (long)slab_word_stride(m); a.sstride = (long)slab_cells(m);
        a.words = z.words + (size_t)kGhost * m->W;
        a.sums = accumulate ? z.sums : nullptr;
        a.cap = z.cap; a.qflux = z.qflux;
        a.C = so.heat_capacity; a.Lv = so.Lv; a.dt = dt;
        a.mask = mask;
        a.W = m->W; a.H = m->H;
        a.j0 = j0; a.n0 = n0; a.jb0 = jb0;
        const dim3 grid((unsigned)((m->W + kSlabLanes - 1) / kSlabLanes), (unsigned)nrows);
        hipLaunchKernelGGL(pe_slab_ocean_kernel, grid, dim3(kSlabLanes), 0, s, a);
        if (hipGetLastError() != hipSuccess) { *err = "hip: slab ocean kernel launch failed"; return GCM_ERR_HIP; }
    }
    if (accumulate) { z.seconds += dt; ++z.n; }
    return GCM_OK;
}

// the registered slab behind the boundary layer of a step: see pe_phase_rows
int pe25d_slab_ocean_rows(Pe25d *m, int j0, int j1, int jb0, int jb1, double dt, bool radiation, bool boundary, bool accumulate,
                          hipStream_t s, std::string *err) {
    if (!m->slab.on) { *err = "slab ocean: not registered (gcm_set_slab_ocean)"; return GCM_ERR_STATE; }
    const int mask = (radiation ? kSlabMaskRadiation : 0) | (boundary ? kSlabMaskBoundary : 0);
    return slab_launch(m, m->slab.par, j0, j1, jb0, jb1, dt, mask, accumulate, s, err);
}

// the words' own rows <-> the host's [GCM_SLAB_WORDS][H][W]
static hipError_t slab_words_copy(Pe25d *m, double *host, const double *in, hipStream_t s) {
    const size_t bytes = sizeof(double) * slab_cells(m);
    hipError_t e = hipSuccess;
    for (int n = 0; n < GCM_SLAB_WORDS && e == hipSuccess; ++n) {
        double *dev = m->slab.words + (size_t)n * slab_word_stride(m) + (size_t)kGhost * m->W;
        e = in ? hipMemcpyAsync(dev, in + (size_t)n * slab_cells(m), bytes, hipMemcpyHostToDevice, s)
               : hipMemcpyAsync(host + (size_t)n * slab_cells(m), dev, bytes, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e;
}

int pe25d_slab_ocean_apply(Pe25d *m, double dt, const gcm_slab_ocean *so, const double *words, hipStream_t s, std::string *err) {
    const char *fn = "gcm_slab_ocean_apply";
    if (int rc = slab_ocean_check(so, fn, err)) return rc;
    if (!std::isfinite(dt) || !words) { *err = std::string(fn) + ": dt must be finite, words are required"; return GCM_ERR_ARG; }
    if (!m->gt_set) { *err = std::string(fn) + ": set the ground temperature first (gcm_set_ground)"; return GCM_ERR_STATE; }
    if (int rc = slab_words_alloc(m, fn, err)) return rc;
    if (int rc = hip_rc(slab_words_copy(m, nullptr, words, s), fn, err)) return rc;
    return slab_launch(m, *so, 0, m->H, 0, 0, dt, kSlabMaskRadiation | kSlabMaskBoundary, m->slab.on, s, err);
}

int pe25d_slab_ocean_fluxes(Pe25d *m, double *words, hipStream_t s, std::string *err) {
    const char *fn = "gcm_get_slab_ocean_fluxes";
    if (!words) { *err = std::string(fn) + ": words are required"; return GCM_ERR_ARG; }
    if (!m->slab.words) { *err = std::string(fn) + ": no slab ocean registered (gcm_set_slab_ocean)"; return GCM_ERR_STATE; }
    return hip_rc(slab_words_copy(m, words, nullptr, s), fn, err);
}

static int slab_registered(const Pe25d *m, const char *fn, std::string *err) {
    if (m->slab.on) return GCM_OK;
    *err = std::string(fn) + ": no slab ocean registered (gcm_set_slab_ocean)";
    return GCM_ERR_STATE;
}

int pe25d_slab_ocean_get(Pe25d *m, double *sums, double *seconds, int64_t *nsteps, hipStream_t s, std::string *err) {
    const char *fn = "gcm_get_slab_ocean";
    if (int rc = slab_registered(m, fn, err)) return rc;
    hipError_t e = hipSuccess;
    if (sums) e = hipMemcpyAsync(sums, m->slab.sums, sizeof(double) * GCM_SLAB_SUMS * slab_cells(m), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (int rc = hip_rc(e, fn, err)) return rc;
    if (seconds) *seconds = m->slab.seconds;
    if (nsteps) *nsteps = m->slab.n;
    return GCM_OK;
}

int pe25d_slab_ocean_put(Pe25d *m, const double *sums, double seconds, int64_t nsteps, hipStream_t s, std::string *err) {
    const char *fn = "gcm_put_slab_ocean";
    if (int rc = slab_registered(m, fn, err)) return rc;
    if (!sums || !std::isfinite(seconds) || seconds < 0.0 || nsteps < 0) {
        *err = std::string(fn) + ": sums are required, seconds must be finite and >= 0, nsteps >= 0";
        return GCM_ERR_ARG;
    }
    hipError_t e = hipMemcpyAsync(m->slab.sums, sums, sizeof(double) * GCM_SLAB_SUMS * slab_cells(m), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);          // (the caller's array is free again when the call returns)
    if (int rc = hip_rc(e, fn, err)) return rc;
    m->slab.seconds = seconds;
    m->slab.n = nsteps;
    return GCM_OK;
}

int pe25d_slab_ocean_reset(Pe25d *m, hipStream_t s, std::string *err) {
    const char *fn = "gcm_slab_ocean_reset";
    if (int rc = slab_registered(m, fn, err)) return rc;
    if (int rc = hip_rc(hipMemsetAsync(m->slab.sums, 0, sizeof(double) * GCM_SLAB_SUMS * slab_cells(m), s), fn, err)) return rc;
    m->slab.seconds = 0.0;
    m->slab.n = 0;
    return GCM_OK;
}

}  // namespace gcm

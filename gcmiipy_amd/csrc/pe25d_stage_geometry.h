// Launch geometry of the GCM_PE25D dynamics stage where it depends on the rows of the launch, the level count, the
// row's filter plan and the chip's compute units: K1, the looping filter kernel (which instantiation, how many
// workgroups a row, how many level pairs each loops over, whether pit rides in the launch) and K4, the row-group update
// kernel (rows per workgroup, row groups, column tiles, the padded grid, the odd-level start).  Host arithmetic only, no
// device: launch_k1, update_rows (pe25d_kernels.hip), pe25d_create (pe25d_state.hip) and the picker
// spu_filter_loop_kernel_for (pe25d_k1.h) take their numbers from here, and so does the query
// gcm_pe25d_stage_geometry / gcm_pe25d_stage_plan (include/gcmcore.h), so that the query cannot drift from the launch.
#pragma once
#include <algorithm>

#include "../../include/gcmcore.h"
#include "fft_lds.h"

namespace gcm {

constexpr int kUpdCols = 62;      // row-group update kernel: columns a wave produces (lanes 0 and 63 carry the halo columns)
// plans with their own instantiation (only their passes compiled in): the row lengths of the
// BASELINE configs and the powers of 16
constexpr unsigned kMask1440 = pass_bit(5, 2) | pass_bit(4, 3);                    // 1440 = 10.12.12, 120 = 10.12
constexpr unsigned kMask2880 = pass_bit(5, 3) | pass_bit(4, 3) | pass_bit(4, 4);   // 2880
constexpr unsigned kMask4096 = pass_bit(4, 4);                                     // 256, 4096

// ---------------------------------------------------------------- K1, the looping form
// The instantiation of pe_spu_filter_loop_kernel<T, MAXR, MASK, NIN, NW> a plan takes; loop == 0: no looping form (K1 as
// one workgroup per level pair).  spu_filter_loop_kernel_for maps this to the kernel, the query reports it.
struct LoopKernelDesc { int loop, maxr; unsigned mask; int nin, nw; };
inline LoopKernelDesc spu_filter_loop_desc(const SuperPlan &P) {
    if (!P.ok || P.npass > 4 || P.npass < 2) return {0, 0, 0u, 0, 0};
    // the plans these masks stand for start with a pass of radix 5.2 / 5.3 / 4.4 (make_super_plan)
    if (P.mask == kMask1440 && P.r1[0] * P.r2[0] == 10 && P.npass <= 3) return {1, 12, kMask1440, 10, 3};
    if (P.mask == kMask2880 && P.r1[0] * P.r2[0] == 15 && P.npass <= 3) return {1, 16, kMask2880, 15, 3};
    if (P.mask == kMask1440) return {1, 12, kMask1440, 12, 5};
    if (P.mask == kMask2880) return {1, 16, kMask2880, 16, 5};
    if (P.mask == kMask4096) return {1, 16, kMask4096, 16, 5};
    if (P.maxr <= 12) return {1, 12, 0u, 12, 5};
    if (P.maxr <= 16) return {1, 16, 0u, 16, 5};
    return {1, 25, 0u, 25, 5};
}
// the row length a mask is named for (the query's k1_mask word), 0: the general form
inline int stage_mask_name(unsigned mask) { return mask == kMask1440 ? 1440 : mask == kMask2880 ? 2880 : mask == kMask4096 ? 4096 : 0; }

// The looping K1 over `rows` rows: all pairs of a row in one workgroup when there are rows enough to fill the chip,
// else groups; ny workgroups a row (one more where pit rides), each loops over ppw pairs, the last over what is left
struct StageK1 { int pairs, groups, ppw, ny; };
inline StageK1 stage_k1_launch(int L, int rows, int cus) {
    const int pairs = (L + 1) / 2;
    const int groups = std::min(pairs, std::max(1, (3 * cus + rows - 1) / rows));
    const int ppw = (pairs + groups - 1) / groups;
    const int ny = (pairs + ppw - 1) / ppw;
    return {pairs, groups, ppw, ny};
}

// ---------------------------------------------------------------- K4
// rows per workgroup (GCM_PE_UPDATE_ROWS overrides it in pe25d_create, where the measurements behind the rule are)
inline int stage_k4_rows(int H, bool f32) { return (H <= 400 || f32) ? 3 : 7; }
// row groups of one launch over n0 + n1 rows in two ranges (the second empty, or a band's other edge)
inline long stage_k4_groups(int n0, int n1, int Rg) { return (std::max(0, n0) + Rg - 1) / Rg + (std::max(0, n1) + Rg - 1) / Rg; }
inline int stage_k4_col_tiles(int W) { return (W + kUpdCols - 1) / kUpdCols; }
// the padded grid: 8 XCDs x (row group, segment) pairs per XCD x column tiles (see the kernel's index map)
inline long stage_k4_grid(long groups, int nseg, int W) {
    const long rs_per_xcd = (groups * nseg + 7) / 8;
    return 8 * rs_per_xcd * stage_k4_col_tiles(W);
}
// whole columns of an even number of levels start on an odd level (see update_rows)
inline bool stage_k4_oddtop(bool enabled, int nseg, int L) { return enabled && nseg == 1 && L % 2 == 0; }

// ---------------------------------------------------------------- the query's words (GCM_STAGE_*)
inline void stage_words_k1(int *o, const SuperPlan &P, bool loop_allowed, int L, int rows, int cus, bool pit2d) {
    const LoopKernelDesc d = loop_allowed ? spu_filter_loop_desc(P) : LoopKernelDesc{0, 0, 0u, 0, 0};
    const int pairs = (L + 1) / 2;
    o[GCM_STAGE_K1_LOOP] = d.loop;
    o[GCM_STAGE_K1_MAXR] = d.maxr;
    o[GCM_STAGE_K1_MASK] = stage_mask_name(d.mask);
    o[GCM_STAGE_K1_NIN] = d.nin;
    o[GCM_STAGE_K1_NW] = d.nw;
    o[GCM_STAGE_K1_PASSES] = P.ok ? P.npass : 0;
    if (d.loop) {
        const StageK1 k = stage_k1_launch(L, rows, cus);
        o[GCM_STAGE_K1_WGS_PER_ROW] = k.ny;
        o[GCM_STAGE_K1_PAIRS_PER_WG] = k.ppw;
        o[GCM_STAGE_K1_PAIRS_LAST_WG] = k.pairs - (k.ny - 1) * k.ppw;
    } else {                                      // one workgroup per level pair
        o[GCM_STAGE_K1_WGS_PER_ROW] = pairs;
        o[GCM_STAGE_K1_PAIRS_PER_WG] = o[GCM_STAGE_K1_PAIRS_LAST_WG] = 1;
    }
    o[GCM_STAGE_K1_PIT_RIDES] = d.loop && pit2d;
}
// K4 over n0 + n1 rows in two ranges: o[0] groups, o[1] rows of the last group, o[2] oddtop, o[3] the padded grid
inline void stage_words_k4_launch(int *o, int W, int n0, int n1, int L, int Rg, int nseg, bool oddtop_enabled) {
    const long groups = stage_k4_groups(n0, n1, Rg);
    const int last = n1 > 0 ? n1 : n0;
    o[0] = (int)groups;
    o[1] = last > 0 ? last - ((last + Rg - 1) / Rg - 1) * Rg : 0;
    o[2] = stage_k4_oddtop(oddtop_enabled, nseg, L);
    o[3] = (int)stage_k4_grid(groups, nseg, W);
}
inline void stage_words_k4(int *o, int W, int rows, int L, int Rg, int nseg, bool oddtop_enabled) {
    int w[4];
    stage_words_k4_launch(w, W, rows, 0, L, Rg, nseg, oddtop_enabled);
    o[GCM_STAGE_K4_ROWS] = Rg;
    o[GCM_STAGE_K4_GROUPS] = w[0];
    o[GCM_STAGE_K4_ROWS_LAST_GROUP] = w[1];
    o[GCM_STAGE_K4_COL_TILES] = stage_k4_col_tiles(W);
    o[GCM_STAGE_K4_COLS_LAST_TILE] = W - (stage_k4_col_tiles(W) - 1) * kUpdCols;
    o[GCM_STAGE_K4_NSEG] = nseg;
    o[GCM_STAGE_K4_ODDTOP] = w[2];
    o[GCM_STAGE_K4_GRID] = w[3];
}

// the words of gcm_filter_plan -> the plan (mask and widest radix from the passes, as make_super_plan forms them)
inline bool stage_plan_of_words(const unsigned *w, int n, SuperPlan *P) {
    *P = SuperPlan{};
    if (n < 3 + 4 * kMaxSuper || w[1] > (unsigned)kMaxSuper) return false;
    P->ok = w[0] != 0;
    P->npass = (int)w[1];
    P->threads = (int)w[2];
    for (int p = 0; p < P->npass; ++p) {
        P->r1[p] = (int)w[3 + 4 * p]; P->r2[p] = (int)w[4 + 4 * p];
        P->magic[p] = w[5 + 4 * p]; P->imagic[p] = w[6 + 4 * p];
        if (P->r1[p] < 1 || P->r2[p] < 1) return false;
        P->maxr = std::max(P->maxr, P->r1[p] * P->r2[p]);
        P->mask |= pass_bit(P->r1[p], P->r2[p]);
    }
    return true;
}

// gcm_pe25d_stage_geometry: a whole-domain stage over `rows` rows at the default switches (pit from the 2-D column
// sums, whole columns, the odd-level start); plan: the words of gcm_filter_plan for W, or null for the library's own
inline int pe25d_stage_geometry(int W, int rows, int L, int cus, int elem_bytes, const unsigned *plan, int nplan, int *out, int nout) {
    if (W < 1 || rows < 1 || L < 1 || cus < 1 || (elem_bytes != 4 && elem_bytes != 8) || !out || nout < GCM_STAGE_PLAN_WORDS)
        return GCM_ERR_ARG;
    SuperPlan P{};
    if (plan) { if (!stage_plan_of_words(plan, nplan, &P)) return GCM_ERR_ARG; }
    else if (W > 1) make_super_plan(W, &P);
    for (int n = 0; n < GCM_STAGE_PLAN_WORDS; ++n) out[n] = 0;
    stage_words_k1(out, P, W > 1, L, rows, cus, true);
    stage_words_k4(out, W, rows, L, stage_k4_rows(rows, elem_bytes == 4), 1, true);
    return GCM_OK;
}

}  // namespace gcm

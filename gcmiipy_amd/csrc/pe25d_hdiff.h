// GCM_PE25D, horizontal diffusion (pe25d_hdiff.hip): the cell routine that host and device share, and the launch
// geometry of the kernel, which gcm_hdiff_plan reports without launching.  The contract: include/gcmcore.h.
#pragma once
#include <cstddef>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace gcm {

// D(X) of one cell from its five values and the three coefficients of its row.  Every operation is an IEEE subtract,
// multiply or add rounded on its own: the units that include this header switch contraction off for the whole file
// (#pragma clang fp contract(off) under -ffp-contract=fast-honor-pragmas), so the host build (gcm_hdiff_apply) and the
// kernel give the same bits.  n: row j - 1, s: row j + 1, w: column i - 1, e: column i + 1
__host__ __device__ inline double hdiff_cell(double c, double w, double e, double n, double s, double ax, double bn, double bs) {
    const double de = e - c;
    const double dw = c - w;
    const double zx = de - dw;
    const double gs = s - c;
    const double gn = c - n;
    const double fx = ax * zx;
    const double fs = bs * gs;
    const double fn = bn * gn;
    const double fy = fs - fn;
    return fx + fy;
}

// ---------------------------------------------------------------- the launch geometry
// A workgroup of kHdThreads takes one level of one field over a tile of kHdRows rows x kHdCols columns.  It loads the
// tile and a halo of `order` cells a side once, widened to float64, into LDS; at order 2 it forms Y = D(X) on the tile
// and one cell a side in a second LDS array; then X' on the tile.  A row is wave-uniform, so the rows' coefficients
// are scalar loads of the device table.
//   LDS at order 2: 8 ((16 + 4)(128 + 4) + (16 + 2)(128 + 2)) = 39840 bytes: four workgroups fit the 160 KB of a CU
//   (two are the floor), 16 waves a CU; at order 1 8 x 18 x 130 = 18720 bytes.
//   Cells loaded per cell written: 20 x 132 / (16 x 128) = 1.29 (order 2), 18 x 130 / 2048 = 1.14 (order 1); the halo
//   rows and columns are another tile's own cells and mostly come from the L2.
//   A row of the LDS arrays is 132 or 130 float64 and a wave reads 64 consecutive ones of it: each half wave covers
//   the 64 banks once, no conflict beyond the two passes an 8-byte read takes anyway.
//   The alternative, a row march with a five-row rolling window per strip, reads no halo rows twice but serialises a
//   strip's rows in one workgroup and needs the window's Y rows in flight as well; the tile was chosen because its
//   redundant reads are 1.29x at the most, every workgroup is independent, and partial tiles need no special path.
constexpr int kHdThreads = 256;
constexpr int kHdRows = 16;
constexpr int kHdCols = 128;
// The band form of the kernel (a latitude band that has opted in, gcm_set_band_hdiff) has the same geometry over the
// band's own rows: its halo rows beyond the own rows are the band's ghost rows, kHdGhost a side -- the radius of order 2
constexpr int kHdGhost = 2;

constexpr size_t hdiff_lds_bytes(int order) {
    return sizeof(double) * ((size_t)(kHdRows + 2 * order) * (kHdCols + 2 * order) +
                             (order == 2 ? (size_t)(kHdRows + 2) * (kHdCols + 2) : 0));
}

struct HdiffGrid { int tiles_i, tiles_j, z; };
inline HdiffGrid hdiff_grid(int W, int H, int L, int nfields) {
    return HdiffGrid{(W + kHdCols - 1) / kHdCols, (H + kHdRows - 1) / kHdRows, nfields * L};
}

}  // namespace gcm

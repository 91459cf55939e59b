// HIP kernels for the 2-D shallow-water family on the doubly periodic C-grid:
//   GCM_SW2D       matsuno_c_grid.matsumo_scheme   (matsuno_c_grid.py:125-142)
//   GCM_SW2D_TEMP  matsumo_temp.matsumo_scheme     (matsumo_temp.py:66-99)
//   tracer         two_d.finite_volume_advection   (two_d.py:198-207) [+ van Leer]
//
// This unit: the float64 instantiation of the kernels (sw2d_impl.h), the Exner table and the
// segment copy of the ghost-row exchange.  The float32 instantiation is sw2d_kernels_f32.hip.
#include "sw2d_kernels.h"

#include <hip/hip_ext.h>

#include <cmath>
#include <cstdlib>

#include "gcm_math.h"
#include "sw2d_impl.h"

namespace gcm {

void build_exner_table(double *tab) {
    const long double kappa = (long double)kKappa, ln2 = logl(2.0L);
    for (int e = -64; e <= 63; ++e)
        tab[e + 64] = (double)expl(kappa * ((long double)e * ln2 - logl((long double)kP0)));
    for (int i = 0; i < 64; ++i) {
        const double rc = (double)(1.0L / (1.0L + ((long double)i + 0.5L) / 64.0L));
        tab[128 + 2 * i] = rc;
        tab[129 + 2 * i] = (double)powl(1.0L / (long double)rc, kappa);
    }
}

GCM_SW2D_INSTANTIATE(double)
// the wave pair: float64 only
template bool launch_sw2d_pair<double>(const Sw2dArgsT<double> &, int, bool, hipStream_t);
template int sw2d_pair_rows_per_band<double>(int, int, int, bool);

__global__ void seg_copy_kernel(SegCopy c) {
    const int seg = blockIdx.y;
    if (seg >= c.nseg) return;
    const long n = c.n[seg];
    const double *src = c.src[seg];
    double *dst = c.dst[seg];
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        dst[i] = src[i];
}

void launch_seg_copy(const SegCopy &c, hipStream_t s, hipEvent_t stop) {
    long mx = 0;
    for (int k = 0; k < c.nseg; ++k) mx = c.n[k] > mx ? c.n[k] : mx;
    if (mx <= 0 || c.nseg <= 0) {
        if (stop) (void)hipEventRecord(stop, s);
        return;
    }
    int blocks = (int)((mx + 255) / 256);
    if (blocks > 512) blocks = 512;
    if (stop) hipExtLaunchKernelGGL(seg_copy_kernel, dim3(blocks, c.nseg), dim3(256), 0, s, nullptr, stop, 0, c);
    else hipLaunchKernelGGL(seg_copy_kernel, dim3(blocks, c.nseg), dim3(256), 0, s, c);
}

}  // namespace gcm

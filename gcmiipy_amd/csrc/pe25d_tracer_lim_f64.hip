// GCM_PE25D, the donor-cell and van Leer limited tracer kernels in double (pe25d_tracer_lim.h)
#include "pe25d_tracer_lim.h"

namespace gcm {
template TracerKernel<double> tracer_lim_kernel_for<double>(int, int, bool);
}  // namespace gcm

// GCM_PE25D, the donor-cell and van Leer limited tracer kernels in float (pe25d_tracer_lim.h)
#include "pe25d_tracer_lim.h"

namespace gcm {
template TracerKernel<float> tracer_lim_kernel_for<float>(int, int, bool);
}  // namespace gcm

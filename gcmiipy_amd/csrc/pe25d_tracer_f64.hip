// GCM_PE25D, the passive-tracer kernel in double (pe25d_tracer.h)
#include "pe25d_tracer.h"

namespace gcm {
template TracerKernel<double> tracer_kernel_for<double>(int, bool);
}  // namespace gcm

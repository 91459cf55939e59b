// GCM_PE25D, the passive-tracer kernel in float (pe25d_tracer.h)
#include "pe25d_tracer.h"

namespace gcm {
template TracerKernel<float> tracer_kernel_for<float>(int, bool);
}  // namespace gcm

// The float32 instantiation of the 2-D shallow-water kernels (sw2d_impl.h), for GCM_F32 handles of GCM_SW2D and
// GCM_SW2D_TEMP: a translation unit of its own, so that the float64 one keeps its compile time and its code
// objects.  Also the conversions between the float64 host arrays and the float32 device state.
#include "sw2d_impl.h"

namespace gcm {

GCM_SW2D_INSTANTIATE(float)

// M slabs of n elements: staging (float64, slab after slab) -> device (float32, slabs `pitch` apart) and back.
// The conversion to float rounds to nearest-even, as np.float32(x) does; the widening is exact.
__global__ __launch_bounds__(256) void narrow_kernel(float *dst, long pitch, const double *src, long n) {
    dst += blockIdx.y * pitch;
    src += blockIdx.y * n;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = (float)src[i];
}
__global__ __launch_bounds__(256) void widen_kernel(double *dst, const float *src, long pitch, long n) {
    dst += blockIdx.y * n;
    src += blockIdx.y * pitch;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = (double)src[i];
}

static dim3 convert_grid(long n, int M) {
    long b = (n + 255) / 256;
    return dim3((unsigned)(b > 1024 ? 1024 : b), (unsigned)M);
}

void launch_narrow(float *dst, long pitch, const double *src, long n, int M, hipStream_t s) {
    if (n <= 0 || M <= 0) return;
    hipLaunchKernelGGL(narrow_kernel, convert_grid(n, M), dim3(256), 0, s, dst, pitch, src, n);
}

void launch_widen(double *dst, const float *src, long pitch, long n, int M, hipStream_t s) {
    if (n <= 0 || M <= 0) return;
    hipLaunchKernelGGL(widen_kernel, convert_grid(n, M), dim3(256), 0, s, dst, src, pitch, n);
}

}  // namespace gcm

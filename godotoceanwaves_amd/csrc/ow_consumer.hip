// ow_consumer.hip -- the read side of the two output arrays, on the device.
//
// What the reference's consumers compute per query point from the RGBA16F layers:
//   water.gdshader:27-39 (vertex)              displacement = sum_i texture(displacements, vec3(UV*scales_i.xy, i)).xyz * scales_i.z
//   water.gdshader:72-82 (fragment)            gradient     = sum_i mix(texture_bicubic, texture, min(1, 0.1 ppm)).xyw * vec3(scales_i.ww, 1)
//                                              (both the bilinear-only sum and the mix with the B-spline filter of :41-68)
//   sea_spray_particle.gdshader:78-96          the spawn mask: unscaled gradient sum -> normal.y window, foam > 0.9
// texture() here is GL_LINEAR + GL_REPEAT on an N x N layer, texel centres at (i + 0.5)/N.  The arithmetic is FP32
// with the weights kept exact (a texture unit quantises them to 8 fractional bits; that is not pinned by the
// reference; the CPU oracle of the test-suite and this kernel both use the exact weights).  This unit is built with
// -ffp-contract=off so that the oracle's restatement of the shaders can be compared with it to the last bit.  The per-point arithmetic
// lives in ow_surface.h, which tests/query/ also compiles as plain C++: k_query_surface is held to that build bit for bit.
#include <hip/hip_runtime.h>

#include "ow_kernels.h"

namespace ow {
namespace {

__global__ void k_sample_surface(const u16x4 *disp, const u16x4 *norm, int n, int cascades, const float *xz, int count,
                                 SurfaceScales scales, SurfaceSample *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    out[i] = sample_point(disp, norm, n, cascades, scales, xz[2 * i], xz[2 * i + 1]);
}

// One lane per query point (ow_surface.h query_point).  A lane leaves the Newton loop when its point has converged; the wave leaves it
// when all of its lanes have.  No LDS: the displacement layers a batch of queries touches stay in the L2 / Infinity Cache.
__global__ void __launch_bounds__(256) k_query_surface(const u16x4 *disp, const u16x4 *norm, int n, int cascades, const float *xz, int count,
                                                       SurfaceScales scales, QueryParams qp, SurfaceQuery *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    out[i] = query_point(disp, norm, n, cascades, scales, qp, xz[2 * i], xz[2 * i + 1]);
}

}  // namespace

hipError_t launch_sample_surface(int n, int cascades, const DeviceBuffers &buf, const float *xz_dev, int count,
                                 const SurfaceScales &scales, SurfaceSample *out_dev, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    const int threads = 256;
    hipLaunchKernelGGL(k_sample_surface, dim3((count + threads - 1) / threads), dim3(threads), 0, s, buf.disp, buf.norm, n, cascades,
                       xz_dev, count, scales, out_dev);
    return hipGetLastError();
}

hipError_t launch_query_surface(int n, int cascades, const DeviceBuffers &buf, const float *xz_dev, int count, const SurfaceScales &scales,
                                const QueryParams &qp, SurfaceQuery *out_dev, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    const int threads = 256;
    hipLaunchKernelGGL(k_query_surface, dim3((count + threads - 1) / threads), dim3(threads), 0, s, buf.disp, buf.norm, n, cascades, xz_dev,
                       count, scales, qp, out_dev);
    return hipGetLastError();
}

}  // namespace ow

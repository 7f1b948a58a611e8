// ow_environment.hip -- the two kernels that finish a picture (ow_environment.h holds the arithmetic, which tests/environment/ also compiles
// as plain C++; the kernels are held to that build bit for bit).  Built with -ffp-contract=off, like ow_solid.hip.
//
//   k_environment_apply  one lane per record: sky fill or fog, color and status rewritten in place
//   k_present<S>         one lane per output pixel: the S x S block of records -> linear float4 and / or the RGBA8 word
//
// HOW A WAVE WALKS THE RECORDS.  A record is one 128-byte line and a lane needs 20 bytes of it (t and status at 0, color at 100), so each
// record costs its whole line whatever the lane order: the only choice is which lines a wave touches together.  Lane l of a wave takes
// record base + l, row-major over the whole picture -- 64 consecutive lines, 8 KiB contiguous per wave, not an 8 x 8 tile's eight 1 KiB
// pieces: nothing here has 2-D reuse (the panorama reads of neighbouring pixels are neighbours either way), and contiguous lines are what
// the memory channels interleave best.  The head is read as one 8-byte vector and (specular, color) as one aligned 16-byte vector;
// the write is that 16-byte vector back (specular's own bits) and the 4-byte status, so a line is read once and written once.
// k_present's lanes run along the OUTPUT row: for each of the S record rows of a block row a wave reads 64 S consecutive records (every
// line of them whole, each by exactly one lane, none twice), and a lane adds its S x S records in row-major order as the definition asks.
// No LDS, no scratch memory, no atomics; neither kernel allocates.
#include <hip/hip_runtime.h>

#include "ow_environment.h"
#include "ow_kernels.h"

namespace ow {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

__global__ void __launch_bounds__(256) k_environment_apply(CameraParams cam, EnvParams ep, RenderPixel *pixels) {
    const uint32_t at = blockIdx.x * 256u + threadIdx.x;  // width x height <= 2^26
    if (at >= (uint32_t)cam.width * (uint32_t)cam.height) return;
    const int j = (int)(at / (uint32_t)cam.width), i = (int)(at - (uint32_t)j * (uint32_t)cam.width);
    char *rec = (char *)(pixels + at);
    const u32x2 head = *(const u32x2 *)rec;                                      // t, status
    u32x4 tail = *(const u32x4 *)(rec + offsetof(RenderPixel, specular));        // specular, color[3]
    const float color[3] = {__uint_as_float(tail.y), __uint_as_float(tail.z), __uint_as_float(tail.w)};
    const EnvPixel px = environment_pixel(ep, cam, i, j, __uint_as_float(head.x), (int32_t)head.y, color);
    if (!px.changed) return;
    tail.y = __float_as_uint(px.color[0]);
    tail.z = __float_as_uint(px.color[1]);
    tail.w = __float_as_uint(px.color[2]);
    *(u32x4 *)(rec + offsetof(RenderPixel, specular)) = tail;
    *(int32_t *)(rec + offsetof(RenderPixel, status)) = px.status;
}

template <int S>
__global__ void __launch_bounds__(256) k_present(int out_width, int out_height, PresentParams pp, const RenderPixel *pixels, uint32_t *rgba, float4 *linear) {
    const uint32_t at = blockIdx.x * 256u + threadIdx.x;
    if (at >= (uint32_t)out_width * (uint32_t)out_height) return;
    const uint32_t oy = at / (uint32_t)out_width, ox = at - oy * (uint32_t)out_width;
    const size_t row_stride = (size_t)out_width * S;
    pp.s = S;  // a constant the loops unroll on; the launcher passes the same value
    float lin[4];
    PresentStages st;
    const uint32_t word = present_pixel(pp, pixels + (size_t)oy * S * row_stride + (size_t)ox * S, row_stride, lin, st);
    if (linear) linear[at] = make_float4(lin[0], lin[1], lin[2], lin[3]);
    if (rgba) rgba[at] = word;
}

}  // namespace

hipError_t launch_environment_apply(const CameraParams &cam, const EnvParams &ep, RenderPixel *pixels_dev, hipStream_t s) {
    static_assert(offsetof(RenderPixel, specular) == 96 && offsetof(RenderPixel, status) == 4 && sizeof(RenderPixel) == 128, "the record's vectors");
    if (cam.width <= 0 || cam.height <= 0 || !pixels_dev || !ep.camera_ok) return hipSuccess;  // a camera that is not finite changes nothing
    const size_t pixels = (size_t)cam.width * cam.height;
    hipLaunchKernelGGL(k_environment_apply, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, s, cam, ep, pixels_dev);
    return hipGetLastError();
}

hipError_t launch_present(int out_width, int out_height, const PresentParams &pp, const RenderPixel *pixels_dev, uint32_t *rgba_dev, float *linear_dev,
                          hipStream_t s) {
    if (out_width <= 0 || out_height <= 0 || (!rgba_dev && !linear_dev)) return hipSuccess;
    const size_t pixels = (size_t)out_width * out_height;
    const dim3 grid((unsigned)((pixels + 255) / 256)), block(256);
    float4 *lin = (float4 *)linear_dev;
    switch (pp.s) {
        case 1: hipLaunchKernelGGL(k_present<1>, grid, block, 0, s, out_width, out_height, pp, pixels_dev, rgba_dev, lin); break;
        case 2: hipLaunchKernelGGL(k_present<2>, grid, block, 0, s, out_width, out_height, pp, pixels_dev, rgba_dev, lin); break;
        case 3: hipLaunchKernelGGL(k_present<3>, grid, block, 0, s, out_width, out_height, pp, pixels_dev, rgba_dev, lin); break;
        case 4: hipLaunchKernelGGL(k_present<4>, grid, block, 0, s, out_width, out_height, pp, pixels_dev, rgba_dev, lin); break;
        default: return hipErrorInvalidValue;  // the host wrappers refuse these first
    }
    return hipGetLastError();
}

}  // namespace ow

// ow_sky_light.hip -- the kernels behind ow_radiance_create and ow_radiance_light_apply (ow_sky_light.h holds the arithmetic, which
// tests/sky_light/ also compiles as plain C++; the kernels are held to that build bit for bit).  Built with -ffp-contract=off, like
// ow_environment.hip.
//
//   k_radiance_decode      one lane per texel of the sky: the decoded texel times the energy, one 16-byte store
//   k_radiance_box         one lane per output texel: the 2 x 2 box of the texture above it
//   k_radiance_prefilter   one lane per texel of R_k: the level's S importance samples of M_k, summed in order on the lane
//   k_radiance_irradiance  one lane per texel of E (512 lanes): the cosine-weighted mean of the chain's small texture, row-major on the lane
//   k_sky_light_apply      one lane per record: ambient and reflection added to color, status marked, in place
//
// The build's lanes run along the row, so neighbouring lanes write neighbouring 16-byte texels and their taps land on neighbouring texels
// of M_k (the sample set is the same for every lane; only the frame turns).  The sample and direction tables are read at addresses that
// are uniform across a wave or consecutive along it.  k_sky_light_apply walks the records as k_environment_apply does: lane l of a wave
// takes record base + l, 64 consecutive 128-byte lines a wave; the head is one 16-byte vector, and a record the pass does not process
// costs no more than that; the others read position, albedo, normal and roughness as the aligned 16-byte vectors that hold them and
// (specular, color) as one, and write that vector back (specular's own bits) and the 4-byte status.  A line is read once and written once.
// No LDS, no scratch memory, no atomics; no kernel allocates.
#include <hip/hip_runtime.h>

#include "ow_kernels.h"
#include "ow_sky_light.h"

namespace ow {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void store_texel(float *out, size_t at, const float v[4]) { ((float4 *)out)[at] = make_float4(v[0], v[1], v[2], v[3]); }

__global__ void __launch_bounds__(256) k_radiance_decode(SprayTexture sky, const float *srgb, float energy, float *out) {
    const uint32_t at = blockIdx.x * 256u + threadIdx.x;  // a side is at most 8192: width x height <= 2^26
    if (at >= (uint32_t)sky.width * (uint32_t)sky.height) return;
    const int j = (int)(at / (uint32_t)sky.width), i = (int)(at - (uint32_t)j * (uint32_t)sky.width);
    float v[4];
    radiance_decode_texel(sky, srgb, energy, i, j, v);
    store_texel(out, at, v);
}

__global__ void __launch_bounds__(256) k_radiance_box(const float *in, int in_width, float *out, int width, int height) {
    const uint32_t at = blockIdx.x * 256u + threadIdx.x;
    if (at >= (uint32_t)width * (uint32_t)height) return;
    const int j = (int)(at / (uint32_t)width), i = (int)(at - (uint32_t)j * (uint32_t)width);
    float v[4];
    radiance_box_texel(in, in_width, i, j, v);
    store_texel(out, at, v);
}

__global__ void __launch_bounds__(256) k_radiance_prefilter(RadianceLevel m, const float *col, const float *row, const float *samples, int S, float *out) {
    const uint32_t at = blockIdx.x * 256u + threadIdx.x;
    if (at >= (uint32_t)m.width * (uint32_t)m.height) return;
    const int j = (int)(at / (uint32_t)m.width), i = (int)(at - (uint32_t)j * (uint32_t)m.width);
    float v[4];
    radiance_prefilter_texel(m, col, row, samples, S, i, j, v);
    store_texel(out, at, v);
}

__global__ void __launch_bounds__(64) k_radiance_irradiance(RadianceLevel m, const float *col, const float *row, const float *ecol, const float *erow, float *out) {
    const uint32_t at = blockIdx.x * 64u + threadIdx.x;
    if (at >= (uint32_t)(kIrradianceWidth * kIrradianceHeight)) return;
    const int j = (int)(at / (uint32_t)kIrradianceWidth), i = (int)(at - (uint32_t)j * (uint32_t)kIrradianceWidth);
    float v[4];
    radiance_irradiance_texel(m, col, row, ecol, erow, i, j, v);
    store_texel(out, at, v);
}

__global__ void __launch_bounds__(256) k_sky_light_apply(CameraParams cam, SkyLightParams lp, RenderPixel *pixels) {
    const uint32_t at = blockIdx.x * 256u + threadIdx.x;  // width x height <= 2^26
    if (at >= (uint32_t)cam.width * (uint32_t)cam.height) return;
    const int j = (int)(at / (uint32_t)cam.width), i = (int)(at - (uint32_t)j * (uint32_t)cam.width);
    char *rec = (char *)(pixels + at);
    const u32x4 head = *(const u32x4 *)rec;  // t, status, position.x, position.y
    const int32_t status = (int32_t)head.y;
    if (!(status & kRayHit) || (status & (kRayEnvironment | kRaySkyLit))) return;
    const u32x4 q1 = *(const u32x4 *)(rec + 16);   // position.z, p, wave_height
    const u32x4 q3 = *(const u32x4 *)(rec + 48);   // foam_factor, albedo
    const u32x4 q4 = *(const u32x4 *)(rec + 64);   // normal, fresnel
    const uint32_t rough = *(const uint32_t *)(rec + offsetof(RenderPixel, roughness));
    u32x4 tail = *(const u32x4 *)(rec + offsetof(RenderPixel, specular));  // specular, color
    const float position[3] = {__uint_as_float(head.z), __uint_as_float(head.w), __uint_as_float(q1.x)};
    const float albedo[3] = {__uint_as_float(q3.y), __uint_as_float(q3.z), __uint_as_float(q3.w)};
    const float normal[3] = {__uint_as_float(q4.x), __uint_as_float(q4.y), __uint_as_float(q4.z)};
    const float color[3] = {__uint_as_float(tail.y), __uint_as_float(tail.z), __uint_as_float(tail.w)};
    const SkyLightPixel px = sky_light_pixel(lp, cam, i, j, status, position, albedo, normal, __uint_as_float(rough), color);
    if (!px.changed) return;
    tail.y = __float_as_uint(px.color[0]);
    tail.z = __float_as_uint(px.color[1]);
    tail.w = __float_as_uint(px.color[2]);
    *(u32x4 *)(rec + offsetof(RenderPixel, specular)) = tail;
    *(int32_t *)(rec + offsetof(RenderPixel, status)) = px.status;
}

dim3 blocks_of(size_t lanes, unsigned block) { return dim3((unsigned)((lanes + block - 1) / block)); }

}  // namespace

hipError_t launch_radiance_build(const RadianceBuild &b, hipStream_t s) {
    const RadiancePlan &p = b.plan;
    // P_0 at the sky's size (M_0 itself where nothing is halved), then the halvings down to M_0
    float *first = p.pre > 0 ? b.pre[0] : b.M[0];
    hipLaunchKernelGGL(k_radiance_decode, blocks_of((size_t)b.sky.width * b.sky.height, 256), dim3(256), 0, s, b.sky, b.srgb, b.energy, first);
    int w = b.sky.width, h = b.sky.height;
    for (int i = 0; i < p.pre; ++i) {
        float *out = i + 1 < p.pre ? b.pre[i + 1] : b.M[0];
        hipLaunchKernelGGL(k_radiance_box, blocks_of((size_t)(w / 2) * (h / 2), 256), dim3(256), 0, s, b.pre[i], w, out, w / 2, h / 2);
        w /= 2;
        h /= 2;
    }
    for (int k = 1; k < p.chain; ++k)
        hipLaunchKernelGGL(k_radiance_box, blocks_of((size_t)p.width[k] * p.height[k], 256), dim3(256), 0, s, b.M[k - 1], p.width[k - 1], b.M[k], p.width[k],
                           p.height[k]);
    for (int k = 1; k < p.levels; ++k) {
        const RadianceLevel m{b.M[k], p.width[k], p.height[k]};
        hipLaunchKernelGGL(k_radiance_prefilter, blocks_of((size_t)m.width * m.height, 256), dim3(256), 0, s, m, b.col[k], b.row[k], b.samples[k], p.samples, b.R[k]);
    }
    const RadianceLevel src{b.M[p.source], p.width[p.source], p.height[p.source]};
    hipLaunchKernelGGL(k_radiance_irradiance, blocks_of((size_t)kIrradianceWidth * kIrradianceHeight, 64), dim3(64), 0, s, src, b.col[p.source], b.row[p.source],
                       b.ecol, b.erow, b.E);
    return hipGetLastError();
}

hipError_t launch_sky_light_apply(const CameraParams &cam, const SkyLightParams &lp, RenderPixel *pixels_dev, hipStream_t s) {
    static_assert(offsetof(RenderPixel, position) == 8 && offsetof(RenderPixel, albedo) == 52 && offsetof(RenderPixel, normal) == 64 &&
                      offsetof(RenderPixel, roughness) == 80 && offsetof(RenderPixel, specular) == 96 && offsetof(RenderPixel, status) == 4 &&
                      sizeof(RenderPixel) == 128,
                  "the record's vectors");
    if (cam.width <= 0 || cam.height <= 0 || !pixels_dev || !lp.camera_ok) return hipSuccess;  // a camera that is not finite changes nothing
    const size_t pixels = (size_t)cam.width * cam.height;
    hipLaunchKernelGGL(k_sky_light_apply, blocks_of(pixels, 256), dim3(256), 0, s, cam, lp, pixels_dev);
    return hipGetLastError();
}

}  // namespace ow

// ow_mist.hip -- the kernel of the height mist (ow_mist.h holds the arithmetic, which tests/mist/ also compiles as plain C++; the kernel is
// held to that build bit for bit).  Built with -ffp-contract=off, like ow_shadow.hip.
//
//   k_mist_apply<kRgba>  one lane per pixel, one 64-lane wave per 8 x 8 tile, as k_shadow_apply: the rays of a tile stay together in the
//                      light's frame, so the lanes of a wave read neighbouring texels of the depth map.  A lane reads its record's first
//                      and seventh 16-byte vectors (t, status; specular, color) and writes those two back; nothing else of the record is
//                      touched.  The slice loop runs mp.slices times in every lane (a kernel argument: the trip count is the wave's);
//                      a lane whose slice lies outside its ray's interval in the frame's box (mist_span) is predicated off for that
//                      trip, and the transmittance is evaluated only at the two boundaries of a shadowed slice.  The map is read with
//                      plain global loads: a 2048^2 map is 16 MB and stays in the Infinity Cache.  No LDS and no scratch memory.
//                      The three counters of a pass are summed across the wave with lane reads; lane 0 adds them with one atomic each
//                      to the block's copy of the counters (kMistCounterSlots copies, a line each: one address would serialise them).
#include <hip/hip_runtime.h>

#include "ow_kernels.h"

namespace ow {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
    return v;
}

template <bool kRgba>
__global__ void __launch_bounds__(64) k_mist_apply(CameraParams cam, MistParams mp, ShadowParams P, const uint32_t *map, int tiles_x, RenderPixel *pixels,
                                                   uint32_t *rgba, unsigned long long *counters) {
    const int lane = (int)threadIdx.x;
    const int tx = (int)blockIdx.x % tiles_x, ty = (int)blockIdx.x / tiles_x;
    const int i = 8 * tx + (lane & 7), j = 8 * ty + (lane >> 3);
    const bool inside = i < cam.width && j < cam.height;
    uint32_t n_pixels = 0u, n_fetched = 0u, n_shadowed = 0u;
    if (inside) {
        const size_t at = (size_t)j * cam.width + i;
        u32x4 *rec = (u32x4 *)(pixels + at);
        u32x4 head = rec[0];                          // t, status, position.xy
        u32x4 tail = rec[6];                          // specular, color
        const float color[3] = {__uint_as_float(tail.y), __uint_as_float(tail.z), __uint_as_float(tail.w)};
        const MistPixel px = mist_pixel(mp, P, map, cam, i, j, __uint_as_float(head.x), (int32_t)head.y, color, true);
        if (px.changed) {
            head.y = (uint32_t)px.status;
            tail.y = __float_as_uint(px.color[0]);
            tail.z = __float_as_uint(px.color[1]);
            tail.w = __float_as_uint(px.color[2]);
            rec[0] = head;
            rec[6] = tail;
            n_pixels = 1u;
            n_fetched = px.fetched;
            n_shadowed = px.shadowed;
        }
        if (kRgba) rgba[at] = pack_rgba8(px.color);
    }
    n_pixels = wave_sum(n_pixels);                    // at most 64, 64 x 256 and 64 x 256
    n_fetched = wave_sum(n_fetched);
    n_shadowed = wave_sum(n_shadowed);
    if (lane == 0 && n_pixels) {
        unsigned long long *slot = counters + (size_t)(blockIdx.x % kMistCounterSlots) * kMistCounterStride;
        atomicAdd(slot + kMistPixels, (unsigned long long)n_pixels);
        if (n_fetched) atomicAdd(slot + kMistFetched, (unsigned long long)n_fetched);
        if (n_shadowed) atomicAdd(slot + kMistShadowed, (unsigned long long)n_shadowed);
    }
}

}  // namespace

hipError_t launch_mist_apply(const uint32_t *map, const CameraParams &cam, const ShadowParams &P, const MistParams &mp, RenderPixel *pixels_dev, uint32_t *rgba_dev,
                             unsigned long long *counters_dev, hipStream_t s) {
    static_assert(offsetof(RenderPixel, specular) == 96 && offsetof(RenderPixel, status) == 4 && sizeof(RenderPixel) == 128, "the record's 16-byte vectors");
    if (cam.width <= 0 || cam.height <= 0 || !pixels_dev || !counters_dev) return hipSuccess;
    if (hipError_t e = hipMemsetAsync(counters_dev, 0, kMistCounterBytes, s); e != hipSuccess) return e;
    if (!mp.camera_ok && !rgba_dev) return hipSuccess;  // nothing would change
    const int tiles_x = (cam.width + 7) / 8, tiles_y = (cam.height + 7) / 8;
    if (rgba_dev)
        hipLaunchKernelGGL(k_mist_apply<true>, dim3(tiles_x * tiles_y), dim3(64), 0, s, cam, mp, P, map, tiles_x, pixels_dev, rgba_dev, counters_dev);
    else
        hipLaunchKernelGGL(k_mist_apply<false>, dim3(tiles_x * tiles_y), dim3(64), 0, s, cam, mp, P, map, tiles_x, pixels_dev, rgba_dev, counters_dev);
    return hipGetLastError();
}

}  // namespace ow

// ow_shadow.hip -- the kernels of the sun shadows (ow_shadow.h holds the arithmetic, which tests/shadow/ also compiles as plain C++; the
// kernels are held to that build bit for bit).  Built with -ffp-contract=off, like ow_solid.hip.
//
//   k_shadow_clear     the map's words to FLT_MAX's bits, the four counters to zero
//   k_shadow_vertices  one lane per (instance, vertex), ow_raster.h's instance_vertices (the vertex stage k_solid_vertices runs): the
//                      instance's transform (a body set's resident pose record, or an uploaded one), the world position, (s, t, d) in the
//                      light's frame, one 16-byte store; vertex 0's lane counts a skipped instance
//   k_shadow_raster    one wave per 64 (instance, triangle) pairs: set-up per lane (facing, the texel box, the class), then ow_raster.h's
//                      raster_wave, the walk k_mesh_raster and k_solid_raster run, into the depth-map target below -- a small box is
//                      walked by its own lane, the large ones are taken one after the other by the whole wave in 8 x 8 tiles, their nine
//                      floats and four integers read from the owning lane (lane reads, no LDS).  A crate face on a 2048^2 map over 100 m
//                      is some 50 texels across: the wave class is the common case
//   k_shadow_apply<kRgba>  one lane per pixel, one wave per 8 x 8 tile (the records are always there; the RGBA8 words are the optional
//                      output): the record's 16-byte vectors that are needed, the taps as plain global loads (neighbouring pixels land on
//                      neighbouring texels only roughly: no tile is staged in LDS), and only the three vectors that hold status, diffuse,
//                      specular and color rewritten, only for receivers
//
// The map is one 32-bit word per texel, the FP32 bits of a depth >= 0, atomicMin on ordinary device memory: the same bytes whatever the
// order of instances, triangles and casts.
#include <hip/hip_runtime.h>

#include "ow_kernels.h"
#include "ow_raster.h"

namespace ow {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void depth_min(uint32_t *map, size_t at, uint32_t bits) {
    // the word only ever decreases (vis_min's argument): a stale read is at worst larger, and then the atomic is merely not spared
    if (bits < map[at]) atomicMin(map + at, bits);
}

// The depth map as raster_wave's target: ShadowSetup's classes (its nine floats and its box are what the wave reads from the owning
// lane), shadow_cover at a texel centre, and the depth's bits written with a min.
struct DepthTarget {
    typedef ShadowSetup Setup;
    float max_depth;
    int size;
    uint32_t *map;
    static constexpr int kLane = kShadowTriLane, kWave = kShadowTriWave;
    __device__ __forceinline__ void centre(const ShadowSetup &S, int i, int j, int) const {
        const ShadowCover c = shadow_cover(S.s, S.t, S.d, max_depth, i, j);
        if (c.hit) depth_min(map, (size_t)j * size + i, c.bits);
    }
};

__global__ void __launch_bounds__(256) k_shadow_clear(uint32_t *map, size_t texels, uint32_t *counters) {
    clear_words(map, texels, kShadowEmpty, counters);
}

__global__ void __launch_bounds__(256) k_shadow_vertices(const float *local, int num_vertices, SolidInstances in, ShadowParams P, ShadowVertex *out,
                                                         uint32_t *counters) {
    instance_vertices(local, num_vertices, in, out, counters + kShadowSkippedInstances, [&](const float *t, bool ok, const float l[3]) { return shadow_vertex(t, ok, l, P); });
}

__global__ void __launch_bounds__(64) k_shadow_raster(const int32_t *indices, int num_vertices, int num_triangles, int num_pairs, const ShadowVertex *verts,
                                                      ShadowParams P, uint32_t *map, uint32_t *counters) {
    const int lane = (int)threadIdx.x;
    const int pair = (int)blockIdx.x * 64 + lane;
    ShadowSetup S;
    __builtin_memset(&S, 0, sizeof(S));
    S.kind = kShadowTriNone;
    if (pair < num_pairs) {
        const SolidTriangle<ShadowVertex> t = solid_triangle(indices, num_vertices, num_triangles, verts, pair);
        S = shadow_setup(*t.a, *t.b, *t.c, P);
    }
    count_classes(counters, lane, S.kind, kShadowTriCulled, kShadowTriWave);  // the class numbers are the counters'
    raster_wave(DepthTarget{P.max_depth, P.size, map}, S, lane, pair, (int)blockIdx.x * 64);
}

// A lane reads 96 of its record's 128 bytes (six vectors) and rewrites 48 of them where the record is a receiver.
template <bool kRgba>
__global__ void __launch_bounds__(64) k_shadow_apply(int width, int height, ShadowParams P, ShadowApply ap, const uint32_t *map, int tiles_x,
                                                     RenderPixel *pixels, uint32_t *rgba) {
    const int lane = (int)threadIdx.x;
    const int tx = (int)blockIdx.x % tiles_x, ty = (int)blockIdx.x / tiles_x;
    const int i = 8 * tx + (lane & 7), j = 8 * ty + (lane >> 3);
    if (i >= width || j >= height) return;
    const size_t at = (size_t)j * width + i;
    typedef RecordWords<RenderPixel> Words;
    Words w;
    u32x4 *rec = (u32x4 *)(pixels + at);
    const u32x4 zero = {0u, 0u, 0u, 0u};
    w.v[2] = w.v[7] = zero;                       // gradient_fragment .. dist and reserved: not read
    w.v[0] = rec[0];                              // t, status, position.xy
    w.v[6] = rec[6];                              // specular, color
    bool changed = false;
    if (shadow_receives(ap, (int32_t)w.v[0].y)) {
        w.v[1] = rec[1];                          // position.z ..
        w.v[3] = rec[3];                          // .. albedo
        w.v[4] = rec[4];                          // normal ..
        w.v[5] = rec[5];                          // .. diffuse
        RenderPixel px = __builtin_bit_cast(RenderPixel, w);
        float V;
        changed = shadow_record(P, ap, map, px, V);
        w = __builtin_bit_cast(Words, px);
    }
    if (changed) {
        rec[0] = w.v[0];
        rec[5] = w.v[5];
        rec[6] = w.v[6];
    }
    if (kRgba) {
        const float color[3] = {__uint_as_float(w.v[6].y), __uint_as_float(w.v[6].z), __uint_as_float(w.v[6].w)};
        rgba[at] = pack_rgba8(color);
    }
}

}  // namespace

hipError_t launch_shadow_clear(const ShadowArrays &A, int size, hipStream_t s) {
    const size_t texels = (size_t)size * size;
    hipLaunchKernelGGL(k_shadow_clear, dim3((unsigned)((texels + 255) / 256)), dim3(256), 0, s, A.map, texels, A.counters);
    return hipGetLastError();
}

hipError_t launch_shadow_cast(const ShadowArrays &A, const SolidInstances &in, const ShadowParams &P, hipStream_t s) {
    const int64_t nverts = (int64_t)in.count * A.shape.num_vertices, npairs = (int64_t)in.count * A.shape.num_triangles;
    if (nverts > kSolidMaxProduct || npairs > kSolidMaxProduct) return hipErrorInvalidValue;  // the host wrappers refuse these first
    if (!P.ok || in.count <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_shadow_vertices, dim3((unsigned)((nverts + 255) / 256)), dim3(256), 0, s, A.shape.local, A.shape.num_vertices, in, P, A.verts, A.counters);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_shadow_raster, dim3((unsigned)((npairs + 63) / 64)), dim3(64), 0, s, A.shape.indices, A.shape.num_vertices, A.shape.num_triangles, (int)npairs, A.verts,
                       P, A.map, A.counters);
    return hipGetLastError();
}

hipError_t launch_shadow_apply(const uint32_t *map, const CameraParams &cam, const ShadowParams &P, const ShadowApply &ap, RenderPixel *pixels_dev,
                               uint32_t *rgba_dev, hipStream_t s) {
    static_assert(offsetof(RenderPixel, specular) == 96 && offsetof(RenderPixel, diffuse) == 84 && offsetof(RenderPixel, normal) == 64 &&
                      offsetof(RenderPixel, albedo) == 52 && sizeof(RenderPixel) == 128,
                  "the record's 16-byte vectors");
    if (cam.width <= 0 || cam.height <= 0 || !pixels_dev) return hipSuccess;
    if ((!P.ok || !ap.camera_ok) && !rgba_dev) return hipSuccess;  // nothing would change
    const int tiles_x = (cam.width + 7) / 8, tiles_y = (cam.height + 7) / 8;
    if (rgba_dev)
        hipLaunchKernelGGL(k_shadow_apply<true>, dim3(tiles_x * tiles_y), dim3(64), 0, s, cam.width, cam.height, P, ap, map, tiles_x, pixels_dev, rgba_dev);
    else
        hipLaunchKernelGGL(k_shadow_apply<false>, dim3(tiles_x * tiles_y), dim3(64), 0, s, cam.width, cam.height, P, ap, map, tiles_x, pixels_dev, rgba_dev);
    return hipGetLastError();
}

}  // namespace ow

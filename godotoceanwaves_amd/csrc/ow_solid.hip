// ow_solid.hip -- the four kernels of a solid draw (ow_solid.h holds the arithmetic, which tests/solid/ also compiles as plain C++; the
// kernels are held to that build bit for bit).  Built with -ffp-contract=off, like ow_mesh.hip.
//
//   k_solid_clear     the visibility buffer to all ones, the four counters to zero
//   k_solid_vertices  one lane per (instance, vertex), ow_raster.h's instance_vertices (the vertex stage k_shadow_vertices runs): the
//                     instance's transform (a body set's resident pose record, or an uploaded one), the world and view positions, a
//                     MeshVertex-compatible record; vertex 0's lane counts a skipped instance
//   k_solid_raster    one wave per 64 (instance, triangle) pairs: set-up per lane (ow_mesh.h tri_setup), then ow_raster.h's raster_wave into
//                     the visibility-buffer target, as k_mesh_raster -- small boxes per lane, large boxes by the whole wave from lane reads
//   k_solid_resolve   one lane per pixel, one wave per 8 x 8 tile: the pixel's word -> barycentrics -> the depth test against the record ->
//                     the shading -> the record (eight 16-byte stores, only where a solid is drawn) and the RGBA8 word (every pixel)
//
// The visibility buffer is k_mesh_raster's: one 64-bit word per pixel, (depth's FP32 bits << 32) | pair, atomicMin on ordinary device
// memory, so the picture is the same bytes on every run.  It lies in the context's own scratch (ow_context::solid), not in the mesh
// draw's.  No LDS, no binning pass.
#include <hip/hip_runtime.h>

#include "ow_kernels.h"
#include "ow_raster.h"

namespace ow {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

__global__ void __launch_bounds__(256) k_solid_clear(uint64_t *vis, size_t pixels, uint32_t *counters) {
    clear_words(vis, pixels, kMeshNoTriangle, counters);
}

__global__ void __launch_bounds__(256) k_solid_vertices(const float *local, int num_vertices, SolidInstances in, CameraParams cam, MeshParams mp,
                                                        MeshVertex *out, uint32_t *counters) {
    instance_vertices(local, num_vertices, in, out, counters + kSolidSkippedInstances, [&](const float *t, bool ok, const float l[3]) { return solid_vertex(t, ok, l, cam, mp); });
}

__global__ void __launch_bounds__(64) k_solid_raster(const int32_t *indices, int num_vertices, int num_triangles, int num_pairs, const MeshVertex *verts,
                                                     CameraParams cam, MeshParams mp, uint64_t *vis, uint32_t *counters) {
    const int lane = (int)threadIdx.x;
    const int pair = (int)blockIdx.x * 64 + lane;
    TriSetup s;
    __builtin_memset(&s, 0, sizeof(s));
    s.kind = -1;
    int counter = -1;
    if (pair < num_pairs) s = solid_setup(solid_triangle(indices, num_vertices, num_triangles, verts, pair), cam, mp, counter);
    for (int k = kSolidCulled; k <= kSolidWave; ++k) {
        const uint64_t m = __ballot(counter == k);
        if (lane == 0 && m) atomicAdd(counters + k, (uint32_t)__popcll(m));
    }
    raster_wave(VisTarget{cam, mp, vis}, s, lane, pair, (int)blockIdx.x * 64);
}

// One lane per pixel, one 8 x 8 tile per wave, as k_mesh_shade.  A lane reads 24 of its record's 128 bytes (t, status; specular, color) and
// rewrites all of them only where a solid is drawn.
template <bool kRecords>
__global__ void __launch_bounds__(64) k_solid_resolve(CameraParams cam, SolidParams sp, const uint64_t *vis, const int32_t *indices, int num_vertices,
                                                      int num_triangles, const MeshVertex *verts, int tiles_x, RenderPixel *pixels, uint32_t *rgba) {
    const int lane = (int)threadIdx.x;
    const int tx = (int)blockIdx.x % tiles_x, ty = (int)blockIdx.x / tiles_x;
    const int i = 8 * tx + (lane & 7), j = 8 * ty + (lane >> 3);
    if (i >= cam.width || j >= cam.height) return;
    const size_t at = (size_t)j * cam.width + i;
    float t = 0.0f, color[3] = {sp.background[0], sp.background[1], sp.background[2]};
    int32_t status = 0;
    if (kRecords) {
        const char *rec = (const char *)(pixels + at);
        const u32x2 head = *(const u32x2 *)rec;                               // t, status
        const u32x4 tail = *(const u32x4 *)(rec + offsetof(RenderPixel, specular));  // specular, color[3]
        t = __uint_as_float(head.x);
        status = (int32_t)head.y;
        color[0] = __uint_as_float(tail.y);
        color[1] = __uint_as_float(tail.z);
        color[2] = __uint_as_float(tail.w);
    }
    bool drawn;
    const RenderPixel px = solid_pixel(sp, cam, vis[at], indices, num_vertices, num_triangles, verts, i, j, t, status, drawn);
    if (drawn) {
        for (int k = 0; k < 3; ++k) color[k] = px.color[k];
        if (kRecords) store_record(pixels + at, px);
    }
    if (rgba) rgba[at] = pack_rgba8(color);
}

}  // namespace

hipError_t launch_solid_draw(const SolidArrays &A, const SolidInstances &in, const CameraParams &cam, const SolidParams &sp, uint32_t *rgba_dev,
                             RenderPixel *pixels_dev, hipStream_t s) {
    static_assert(offsetof(RenderPixel, specular) == 96 && sizeof(RenderPixel) % 16 == 0, "the record's 16-byte vectors");
    if (cam.width <= 0 || cam.height <= 0 || (!rgba_dev && !pixels_dev)) return hipSuccess;
    const size_t pixels = (size_t)cam.width * cam.height;
    hipLaunchKernelGGL(k_solid_clear, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, s, A.vis, pixels, A.counters);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    const int64_t nverts = (int64_t)in.count * A.shape.num_vertices, npairs = (int64_t)in.count * A.shape.num_triangles;
    if (nverts > kSolidMaxProduct || npairs > kSolidMaxProduct) return hipErrorInvalidValue;  // the host wrappers refuse these first
    if (sp.mp.camera_ok && in.count > 0) {  // a camera that is not finite draws nothing: the counters stay 0
        hipLaunchKernelGGL(k_solid_vertices, dim3((unsigned)((nverts + 255) / 256)), dim3(256), 0, s, A.shape.local, A.shape.num_vertices, in, cam, sp.mp, A.verts,
                           A.counters);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        hipLaunchKernelGGL(k_solid_raster, dim3((unsigned)((npairs + 63) / 64)), dim3(64), 0, s, A.shape.indices, A.shape.num_vertices, A.shape.num_triangles, (int)npairs,
                           A.verts, cam, sp.mp, A.vis, A.counters);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    const int tiles_x = (cam.width + 7) / 8, tiles_y = (cam.height + 7) / 8;
    if (pixels_dev)
        hipLaunchKernelGGL(k_solid_resolve<true>, dim3(tiles_x * tiles_y), dim3(64), 0, s, cam, sp, A.vis, A.shape.indices, A.shape.num_vertices, A.shape.num_triangles,
                           A.verts, tiles_x, pixels_dev, rgba_dev);
    else
        hipLaunchKernelGGL(k_solid_resolve<false>, dim3(tiles_x * tiles_y), dim3(64), 0, s, cam, sp, A.vis, A.shape.indices, A.shape.num_vertices, A.shape.num_triangles,
                           A.verts, tiles_x, pixels_dev, rgba_dev);
    return hipGetLastError();
}

}  // namespace ow

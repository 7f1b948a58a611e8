// ow_mesh.hip -- the four kernels of a mesh draw (ow_mesh.h holds the arithmetic, which tests/mesh/ also compiles as plain C++; the
// kernels are held to that build bit for bit).  Built with -ffp-contract=off, like ow_consumer.hip.
//
//   k_mesh_vertices  one lane per vertex: water.gdshader's vertex(), one displacement tap per cascade, the view transform, the record
//   k_mesh_clear     the visibility buffer to all ones, the four counters to zero
//   k_mesh_raster    one wave per 64 triangles: set-up per lane, small boxes per lane, large boxes by the whole wave (below)
//   k_mesh_shade     one lane per pixel, one wave per 8 x 8 tile: the pixel's word -> barycentrics -> varyings -> fragment(), light()
//
// The visibility buffer is one 64-bit word per pixel, (depth's FP32 bits << 32) | triangle index, written with atomicMin on ordinary
// device memory: a positive float's bits are monotone in its value and a min does not depend on the order, so the picture is the same
// bits on every run.  No LDS, no binning pass, no scratch memory (profiles/mesh_kernels_isa.txt).
#include <hip/hip_runtime.h>

#include "ow_kernels.h"
#include "ow_raster.h"

namespace ow {
namespace {

__global__ void __launch_bounds__(256) k_mesh_vertices(const u16x4 *disp, int n, int cascades, const float *local, int count, SurfaceScales scales,
                                                       MeshParams mp, CameraParams cam, int has_camera, float ox, float oy, float oz,
                                                       MeshVertex *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float l[3] = {local[3 * (size_t)i], local[3 * (size_t)i + 1], local[3 * (size_t)i + 2]}, origin[3] = {ox, oy, oz};
    store_record(out + i, mesh_vertex(disp, n, cascades, scales, mp, cam, has_camera != 0, l, origin));
}

__global__ void __launch_bounds__(256) k_mesh_clear(uint64_t *vis, size_t pixels, uint32_t *counters) {
    clear_words(vis, pixels, kMeshNoTriangle, counters);
}

// One 64-lane wave per 64 triangles, one wave per block.  A clipmap seen from eye height has triangles hundreds of pixels wide beside the
// camera and sub-pixel ones towards the horizon in the same draw: each lane sets its own triangle up (tri_setup: class, planes, pixel
// box); a lane whose box is at most lane_box centres a side walks it alone; the triangles with larger boxes are found by a ballot and
// taken one after the other by the whole wave, their planes and box read from the owning lane (the source lane is wave-uniform: a lane
// read, no LDS), the 64 lanes sweeping the box in 8 x 8 tiles: ow_raster.h's raster_wave into the visibility-buffer target, the walk
// k_solid_raster and k_shadow_raster run.  The four classes are counted per wave and added once.
__global__ void __launch_bounds__(64) k_mesh_raster(const int32_t *indices, int num_triangles, const MeshVertex *verts, CameraParams cam, MeshParams mp,
                                                    uint64_t *vis, uint32_t *counters) {
    const int lane = (int)threadIdx.x;
    const int tri = (int)blockIdx.x * 64 + lane;
    TriSetup s;
    __builtin_memset(&s, 0, sizeof(s));
    s.kind = -1;
    if (tri < num_triangles) {
        const int32_t ia = indices[3 * (size_t)tri], ib = indices[3 * (size_t)tri + 1], ic = indices[3 * (size_t)tri + 2];
        s = tri_setup(verts[ia], verts[ib], verts[ic], cam, mp);
    }
    for (int k = 0; k < 4; ++k) {
        const uint64_t m = __ballot(s.kind == k);
        if (lane == 0 && m) atomicAdd(counters + k, (uint32_t)__popcll(m));
    }
    raster_wave(VisTarget{cam, mp, vis}, s, lane, tri, (int)blockIdx.x * 64);
}

// One lane per pixel, one 8 x 8 tile per wave, as k_render_view: lane l is pixel (8 tx + (l & 7), 8 ty + (l >> 3)).  The barycentrics come
// from tri_planes / tri_cover, the functions the raster kernel called.
template <bool kRecords>
__global__ void __launch_bounds__(64) k_mesh_shade(const u16x4 *disp, const u16x4 *norm, int n, int cascades, SurfaceScales scales, CameraParams cam,
                                                   ShadeParams sp, MeshParams mp, const uint64_t *vis, const int32_t *indices, const MeshVertex *verts,
                                                   int tiles_x, uint32_t *rgba, RenderPixel *pixels) {
    const int lane = (int)threadIdx.x;
    const int tx = (int)blockIdx.x % tiles_x, ty = (int)blockIdx.x / tiles_x;
    const int i = 8 * tx + (lane & 7), j = 8 * ty + (lane >> 3);
    if (i >= cam.width || j >= cam.height) return;
    const size_t at = (size_t)j * cam.width + i;
    uint32_t word;
    const RenderPixel px = mesh_pixel(disp, norm, n, cascades, scales, cam, sp, mp, vis[at], indices, verts, i, j, &word);
    if (rgba) rgba[at] = word;
    if (kRecords) store_record(pixels + at, px);
}

}  // namespace

hipError_t launch_mesh_vertices(int n, int cascades, const DeviceBuffers &buf, const MeshArrays &M, const SurfaceScales &scales, const MeshParams &mp,
                                const CameraParams &cam, bool has_camera, const float origin[3], hipStream_t s) {
    if (M.num_vertices <= 0) return hipSuccess;
    const int threads = 256;
    hipLaunchKernelGGL(k_mesh_vertices, dim3((M.num_vertices + threads - 1) / threads), dim3(threads), 0, s, buf.disp, n, cascades, M.local,
                       M.num_vertices, scales, mp, cam, has_camera ? 1 : 0, origin[0], origin[1], origin[2], M.verts);
    return hipGetLastError();
}

hipError_t launch_mesh_draw(int n, int cascades, const DeviceBuffers &buf, const MeshArrays &M, const SurfaceScales &scales, const MeshParams &mp,
                            const CameraParams &cam, const ShadeParams &sp, const float origin[3], uint64_t *vis_dev, uint32_t *rgba_dev,
                            RenderPixel *pixels_dev, hipStream_t s) {
    if (cam.width <= 0 || cam.height <= 0 || (!rgba_dev && !pixels_dev)) return hipSuccess;
    if (hipError_t e = launch_mesh_vertices(n, cascades, buf, M, scales, mp, cam, true, origin, s); e != hipSuccess) return e;
    const size_t pixels = (size_t)cam.width * cam.height;
    hipLaunchKernelGGL(k_mesh_clear, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, s, vis_dev, pixels, M.counters);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_mesh_raster, dim3((M.num_triangles + 63) / 64), dim3(64), 0, s, M.indices, M.num_triangles, M.verts, cam, mp, vis_dev, M.counters);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    const int tiles_x = (cam.width + 7) / 8, tiles_y = (cam.height + 7) / 8;
    if (pixels_dev)
        hipLaunchKernelGGL(k_mesh_shade<true>, dim3(tiles_x * tiles_y), dim3(64), 0, s, buf.disp, buf.norm, n, cascades, scales, cam, sp, mp, vis_dev,
                           M.indices, M.verts, tiles_x, rgba_dev, pixels_dev);
    else
        hipLaunchKernelGGL(k_mesh_shade<false>, dim3(tiles_x * tiles_y), dim3(64), 0, s, buf.disp, buf.norm, n, cascades, scales, cam, sp, mp, vis_dev,
                           M.indices, M.verts, tiles_x, rgba_dev, pixels_dev);
    return hipGetLastError();
}

}  // namespace ow

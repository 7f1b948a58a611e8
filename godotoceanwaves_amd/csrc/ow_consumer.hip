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

#include <algorithm>

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

// One lane per hull point (ow_buoyancy.h buoyancy_point), the shape of k_query_surface: a lane's cost is the dependent chain of its Newton
// iterations, which the warm start shortens.  The lane reads its own previous record before it overwrites it.
__global__ void __launch_bounds__(256) k_buoyancy_points(const u16x4 *disp, int n, int cascades, const BuoyancyBody *bodies, int num_bodies,
                                                         const HullPoint *hull, int num_points, SurfaceScales scales, QueryParams qp,
                                                         BuoyancyParams bp, BuoyancyPoint *pts) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_points) return;
    BuoyancyPoint prev;
    if (bp.warm_start) {
        prev = pts[i];
    } else {
        prev.world[0] = prev.world[2] = prev.p[0] = prev.p[1] = 0.0f;
        prev.converged = 0;
    }
    pts[i] = buoyancy_point(disp, n, cascades, scales, qp, bp, bodies, num_bodies, hull, i, prev);
}

// k_buoyancy_points with OW_BUOYANCY_WATER_VELOCITY: the drag is taken relative to the surface's velocity (ow_velocity.h)
__global__ void __launch_bounds__(256) k_buoyancy_points_moving(const u16x4 *disp, const u16x4 *vel, int n, int cascades, const BuoyancyBody *bodies,
                                                                int num_bodies, const HullPoint *hull, int num_points, SurfaceScales scales,
                                                                QueryParams qp, BuoyancyParams bp, BuoyancyPoint *pts) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_points) return;
    BuoyancyPoint prev;
    if (bp.warm_start) {
        prev = pts[i];
    } else {
        prev.world[0] = prev.world[2] = prev.p[0] = prev.p[1] = 0.0f;
        prev.converged = 0;
    }
    pts[i] = buoyancy_point_moving(disp, vel, n, cascades, scales, qp, bp, bodies, num_bodies, hull, i, prev);
}

// One lane per query point (ow_velocity.h velocity_point), the shape of k_query_surface
__global__ void __launch_bounds__(256) k_query_velocity(const u16x4 *disp, const u16x4 *vel, int n, int cascades, const float *xz, int count,
                                                        SurfaceScales scales, QueryParams qp, SurfaceVelocity *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    out[i] = velocity_point(disp, vel, n, cascades, scales, qp, xz[2 * i], xz[2 * i + 1]);
}

__device__ inline BodySum shfl_xor_sum(const BodySum &a, int m) {
    BodySum o;
    for (int k = 0; k < 3; ++k) {
        o.F[k] = __shfl_xor(a.F[k], m, 64);
        o.T[k] = __shfl_xor(a.T[k], m, 64);
        o.M[k] = __shfl_xor(a.M[k], m, 64);
    }
    o.SV = __shfl_xor(a.SV, m, 64);
    o.wetted = __shfl_xor(a.wetted, m, 64);
    o.unconverged = __shfl_xor(a.unconverged, m, 64);
    o.invalid = __shfl_xor(a.invalid, m, 64);
    o.max_residual = __shfl_xor(a.max_residual, m, 64);
    return o;
}

// One 64-lane wave per body, four bodies per block: the lanes sum the body's records in the order ow_buoyancy.h fixes, then the xor tree
// 32, 16, 8, 4, 2, 1 combines them; lane 0 writes the result.
__global__ void __launch_bounds__(256) k_buoyancy_bodies(const BuoyancyBody *bodies, int num_bodies, const HullPoint *hull, int num_points,
                                                         const BuoyancyPoint *pts, BuoyancyResult *results) {
    const int bi = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    if (bi >= num_bodies) return;  // wave-uniform
    const BuoyancyBody b = bodies[bi];
    BodySum a = body_sum_lane(b, bi, hull, pts, num_points, lane);
    for (int m = 32; m >= 1; m >>= 1) a = body_sum_combine(a, shfl_xor_sum(a, m));
    if (lane == 0) results[bi] = body_result(a, b);
}

// ---- floating bodies (ow_rigid.h) ------------------------------------------------------------------------------------------------------
// Fused: one 64-lane wave per body, four bodies per block, the shape of k_buoyancy_bodies, all substeps of the call inside the kernel.  The
// wave keeps the body's FP64 state in registers; per substep every lane forms the pose record (lane 0 writes it), evaluates its hull points
// and adds them up as it goes (rigid_lane: body_sum_lane's order), the xor tree leaves the sums in every lane, and every lane integrates the
// same state from them: nothing is broadcast and nothing but the lane's own point records is read back from memory.  Bodies do not interact:
// no synchronisation beyond the wave's shuffles.
template <bool Moving>
__global__ void __launch_bounds__(256) k_bodies_step(const u16x4 *disp, const u16x4 *vel, int n, int cascades, BodiesArrays A, SurfaceScales scales,
                                                     QueryParams qp, BuoyancyParams bp, RigidParams rp, int substeps) {
    const int bi = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    if (bi >= A.num_bodies) return;  // wave-uniform
    RigidBody s = A.state[bi];
    int32_t flag = A.flags[bi];
    for (int step = 0; step < substeps; ++step) {
        const bool ok = rigid_ok(s);
        const BuoyancyBody b = rigid_pose(s, ok);
        if (lane == 0) A.records[bi] = b;
        BodySum a;
        if constexpr (Moving) {
            const MovingWater water{vel, n, cascades, &scales};
            a = rigid_lane(disp, n, cascades, scales, qp, bp, b, bi, s.point_offset, s.point_count, A.hull, A.pts, A.num_points, lane, water);
        } else {
            a = rigid_lane(disp, n, cascades, scales, qp, bp, b, bi, s.point_offset, s.point_count, A.hull, A.pts, A.num_points, lane, StillWater{});
        }
        for (int m = 32; m >= 1; m >>= 1) a = body_sum_combine(a, shfl_xor_sum(a, m));
        const BuoyancyResult r = rigid_finish(s, ok, flag, a, b, rp);
        if (lane == 0 && step == substeps - 1) A.results[bi] = r;
    }
    if (lane == 0) {
        A.records[bi] = rigid_pose(s, rigid_ok(s));  // the pose after the last substep
        A.state[bi] = s;
        A.flags[bi] = flag;
    }
}

// Split: k_buoyancy_bodies plus the integration and the next pose record, behind a k_buoyancy_points[_moving] launch over the set's points.
__global__ void __launch_bounds__(256) k_bodies_integrate(BodiesArrays A, RigidParams rp) {
    const int bi = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    if (bi >= A.num_bodies) return;  // wave-uniform
    const BuoyancyBody b = A.records[bi];
    RigidBody s = A.state[bi];
    int32_t flag = A.flags[bi];
    BodySum a = body_sum_lane(b, bi, A.hull, A.pts, A.num_points, lane);
    for (int m = 32; m >= 1; m >>= 1) a = body_sum_combine(a, shfl_xor_sum(a, m));
    const BuoyancyResult r = rigid_finish(s, rigid_ok(s), flag, a, b, rp);
    if (lane == 0) {
        A.results[bi] = r;
        A.records[bi] = rigid_pose(s, rigid_ok(s));
        A.state[bi] = s;
        A.flags[bi] = flag;
    }
}

// The pose records of bodies [first, first + count) from their states, their fault flags lowered and their point records zeroed (a cold
// start): after ow_bodies_create and ow_bodies_set_state.  One wave per body.
__global__ void __launch_bounds__(256) k_bodies_pose(BodiesArrays A, int first, int count) {
    const int k = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    if (k >= count) return;  // wave-uniform
    const int bi = first + k;
    const RigidBody s = A.state[bi];
    const int64_t off = s.point_offset, end = off + (int64_t)(s.point_count > 0 ? s.point_count : 0);
    const int64_t lo = off > 0 ? off : 0, hi = end < (int64_t)A.num_points ? end : (int64_t)A.num_points;
    BuoyancyPoint zero = invalid_point();
    zero.body = 0;
    for (int64_t i = lo + lane; i < hi; i += 64) A.pts[i] = zero;
    if (lane == 0) {
        A.records[bi] = rigid_pose(s, rigid_ok(s));
        A.flags[bi] = 0;
    }
}

// Step 1 of a ray cast (ow_raycast.h): the largest FP16 magnitude of D_y per cascade, as bits, into bound[c], which the caller clears in
// stream order before the launch.  blockIdx.y is the cascade; a grid-stride loop reads two texels (16 B) per lane and step, the wave's
// max goes out in one atomicMax.  A max of integers: the same bits in any order.
__global__ void __launch_bounds__(256) k_height_bound(const u16x4 *disp, int n, uint32_t *bound) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const int c = blockIdx.y;
    const size_t pairs = (size_t)n * n / 2;
    const u32x4 *layer = (const u32x4 *)(disp + (size_t)c * n * n);
    uint32_t m = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < pairs; i += (size_t)gridDim.x * blockDim.x) {
        const u32x4 v = layer[i];  // (x, y) (z, w) of texel 2i, then of texel 2i + 1: D_y is the high half of words 0 and 2
        const uint32_t a = (v.x >> 16) & 0x7fffu, b = (v.z >> 16) & 0x7fffu;
        m = max(m, max(a, b));
    }
    for (int s = 32; s >= 1; s >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, s, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(bound + c, m);
}

// the 64 lanes of one wave as ow_raycast.h's raycast_ray sees them: lane j evaluates its own sample; ballots and shuffles make the
// outcome of a round wave-uniform
struct DeviceWave {
    int lane;
    float my_t = 0.0f, my_g = 0.0f;
    template <class Pred, class Fn>
    __device__ void round(const Pred &pred, const Fn &fn, uint64_t &took, uint64_t &above) {
        const bool p = pred(lane);
        RaySample s{0.0f, 0.0f, 0.0f};
        if (p) s = fn(lane);
        my_t = s.t;
        my_g = s.g;
        took = __ballot(p);
        above = __ballot(p && s.g > 0.0f);
    }
    __device__ float t(int j) const { return __shfl(my_t, j, 64); }
    __device__ float g(int j) const { return __shfl(my_g, j, 64); }
};

// One 64-lane wave per ray, one ray per block of 64, no LDS.  Lane j takes sample 64 r + j of round r, each with its own cold solve:
// a ray costs about one dependent-load chain per round (one march round for a steep ray, up to four refine rounds and the record)
// instead of one per sample.  64-thread blocks spread a few rays over as many CUs (a 256-thread block would put four rays on one CU and
// leave the rest of the chip idle); tens of thousands of rays still fill every SIMD.  Lane 0 writes the record.
__global__ void __launch_bounds__(64) k_raycast_surface(const u16x4 *disp, const u16x4 *norm, int n, int cascades, const Ray *rays,
                                                        const uint32_t *bound, SurfaceScales scales, RaycastParams rp, RaycastHit *out) {
    const int i = blockIdx.x;
    DeviceWave wave;
    wave.lane = (int)threadIdx.x;
    const float hw = slab_half_height(bound, cascades, scales);
    const RaycastHit h = raycast_ray(wave, disp, norm, n, cascades, scales, rp, rays[i], hw);
    if (wave.lane == 0) out[i] = h;
}

// One 64-lane wave per 8 x 8 pixel tile of a camera view (ow_render.h), one lane per pixel, one tile per block of 64, no LDS: lane l is
// pixel (8 tx + (l & 7), 8 ty + (l >> 3)).  Each lane marches its own ray sample by sample (march_pixel: the ray cast's samples in order,
// up to the first class change), embeds the query at the hit and shades it.  Neighbouring rays leave the slab after nearly the same number
// of samples, so a wave stays converged but for tiles the horizon crosses; lanes outside the image are inactive.  The record leaves as
// eight 16-byte vector stores and the RGBA8 pixel as one word.  __launch_bounds__(64) states the block size and asks for no occupancy: the
// kernel is a chain of dependent loads per sample, hidden by waves per SIMD, and the compiler's own allocation is 96 VGPRs -- 5 waves per
// SIMD -- with no scratch (profiles/render_view_1024x4.txt); the measured limit is the longest lane's chain, not residency.
template <bool kRecords>
__global__ void __launch_bounds__(64) k_render_view(const u16x4 *disp, const u16x4 *norm, int n, int cascades, const uint32_t *bound,
                                                    SurfaceScales scales, RaycastParams rp, CameraParams cam, ShadeParams sp, int tiles_x,
                                                    uint32_t *rgba, RenderPixel *pixels) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const int lane = (int)threadIdx.x;
    const int tx = (int)blockIdx.x % tiles_x, ty = (int)blockIdx.x / tiles_x;
    const int i = 8 * tx + (lane & 7), j = 8 * ty + (lane >> 3);
    if (i >= cam.width || j >= cam.height) return;
    const float hw = slab_half_height(bound, cascades, scales);
    uint32_t word;
    const RenderPixel px = render_pixel(disp, norm, n, cascades, scales, rp, cam, sp, hw, i, j, &word);
    const size_t at = (size_t)j * cam.width + i;
    if (rgba) rgba[at] = word;
    if (kRecords) {
        struct Words {
            u32x4 v[sizeof(RenderPixel) / 16];
        };
        const Words w = __builtin_bit_cast(Words, px);
        u32x4 *dst = (u32x4 *)(pixels + at);
        for (int k = 0; k < (int)(sizeof(RenderPixel) / 16); ++k) dst[k] = w.v[k];
    }
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

hipError_t launch_buoyancy(int n, int cascades, const DeviceBuffers &buf, const BuoyancyBody *bodies_dev, int num_bodies, const HullPoint *hull_dev,
                           int num_points, const SurfaceScales &scales, const QueryParams &qp, const BuoyancyParams &bp, BuoyancyPoint *pts_dev,
                           BuoyancyResult *results_dev, hipStream_t s, const u16x4 *vel) {
    const int threads = 256;
    if (num_points > 0) {
        if (vel)
            hipLaunchKernelGGL(k_buoyancy_points_moving, dim3((num_points + threads - 1) / threads), dim3(threads), 0, s, buf.disp, vel, n, cascades,
                               bodies_dev, num_bodies, hull_dev, num_points, scales, qp, bp, pts_dev);
        else
            hipLaunchKernelGGL(k_buoyancy_points, dim3((num_points + threads - 1) / threads), dim3(threads), 0, s, buf.disp, n, cascades, bodies_dev,
                               num_bodies, hull_dev, num_points, scales, qp, bp, pts_dev);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    if (num_bodies > 0) {
        hipLaunchKernelGGL(k_buoyancy_bodies, dim3((num_bodies + 3) / 4), dim3(threads), 0, s, bodies_dev, num_bodies, hull_dev, num_points,
                           pts_dev, results_dev);
        return hipGetLastError();
    }
    return hipSuccess;
}

hipError_t launch_bodies_pose(const BodiesArrays &A, int first, int count, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_bodies_pose, dim3((count + 3) / 4), dim3(256), 0, s, A, first, count);
    return hipGetLastError();
}

hipError_t launch_bodies_step(int n, int cascades, const DeviceBuffers &buf, const BodiesArrays &A, const SurfaceScales &scales, const QueryParams &qp,
                              const BuoyancyParams &bp, const RigidParams &rp, int substeps, bool fused, hipStream_t s, const u16x4 *vel) {
    if (A.num_bodies <= 0 || substeps <= 0) return hipSuccess;
    const int threads = 256;
    const dim3 body_grid((A.num_bodies + 3) / 4);
    if (fused) {
        if (vel)
            hipLaunchKernelGGL(k_bodies_step<true>, body_grid, dim3(threads), 0, s, buf.disp, vel, n, cascades, A, scales, qp, bp, rp, substeps);
        else
            hipLaunchKernelGGL(k_bodies_step<false>, body_grid, dim3(threads), 0, s, buf.disp, vel, n, cascades, A, scales, qp, bp, rp, substeps);
        return hipGetLastError();
    }
    for (int step = 0; step < substeps; ++step) {
        if (A.num_points > 0) {
            const dim3 point_grid((A.num_points + threads - 1) / threads);
            if (vel)
                hipLaunchKernelGGL(k_buoyancy_points_moving, point_grid, dim3(threads), 0, s, buf.disp, vel, n, cascades, A.records, A.num_bodies, A.hull,
                                   A.num_points, scales, qp, bp, A.pts);
            else
                hipLaunchKernelGGL(k_buoyancy_points, point_grid, dim3(threads), 0, s, buf.disp, n, cascades, A.records, A.num_bodies, A.hull, A.num_points,
                                   scales, qp, bp, A.pts);
            if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k_bodies_integrate, body_grid, dim3(threads), 0, s, A, rp);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_query_velocity(int n, int cascades, const DeviceBuffers &buf, const u16x4 *vel, const float *xz_dev, int count,
                                 const SurfaceScales &scales, const QueryParams &qp, SurfaceVelocity *out_dev, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    const int threads = 256;
    hipLaunchKernelGGL(k_query_velocity, dim3((count + threads - 1) / threads), dim3(threads), 0, s, buf.disp, vel, n, cascades, xz_dev, count,
                       scales, qp, out_dev);
    return hipGetLastError();
}

hipError_t launch_raycast(int n, int cascades, const DeviceBuffers &buf, const Ray *rays_dev, int count, const SurfaceScales &scales,
                          const RaycastParams &rp, uint32_t *bound_dev, RaycastHit *out_dev, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    if (hipError_t e = hipMemsetAsync(bound_dev, 0, (size_t)cascades * sizeof(uint32_t), s); e != hipSuccess) return e;
    const int threads = 256;
    const int pairs = n * n / 2, blocks = std::min((pairs + threads - 1) / threads, 256);
    hipLaunchKernelGGL(k_height_bound, dim3(blocks, cascades), dim3(threads), 0, s, buf.disp, n, bound_dev);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_raycast_surface, dim3(count), dim3(64), 0, s, buf.disp, buf.norm, n, cascades, rays_dev, bound_dev, scales, rp, out_dev);
    return hipGetLastError();
}

hipError_t launch_render_view(int n, int cascades, const DeviceBuffers &buf, const CameraParams &cam, const SurfaceScales &scales,
                              const RaycastParams &rp, const ShadeParams &sp, uint32_t *bound_dev, uint32_t *rgba_dev, RenderPixel *pixels_dev,
                              hipStream_t s) {
    if (cam.width <= 0 || cam.height <= 0 || (!rgba_dev && !pixels_dev)) return hipSuccess;
    if (hipError_t e = hipMemsetAsync(bound_dev, 0, (size_t)cascades * sizeof(uint32_t), s); e != hipSuccess) return e;
    const int threads = 256;
    const int pairs = n * n / 2, blocks = std::min((pairs + threads - 1) / threads, 256);
    hipLaunchKernelGGL(k_height_bound, dim3(blocks, cascades), dim3(threads), 0, s, buf.disp, n, bound_dev);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    const int tiles_x = (cam.width + 7) / 8, tiles_y = (cam.height + 7) / 8;
    if (pixels_dev)
        hipLaunchKernelGGL(k_render_view<true>, dim3(tiles_x * tiles_y), dim3(64), 0, s, buf.disp, buf.norm, n, cascades, bound_dev, scales, rp, cam,
                           sp, tiles_x, rgba_dev, pixels_dev);
    else
        hipLaunchKernelGGL(k_render_view<false>, dim3(tiles_x * tiles_y), dim3(64), 0, s, buf.disp, buf.norm, n, cascades, bound_dev, scales, rp, cam,
                           sp, tiles_x, rgba_dev, pixels_dev);
    return hipGetLastError();
}

}  // namespace ow

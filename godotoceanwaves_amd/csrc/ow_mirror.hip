// ow_mirror.hip -- the kernel of the floating bodies' reflections (ow_mirror.h holds the arithmetic, which tests/mirror/ also compiles as
// plain C++; the kernel is held to that build bit for bit).  Built with -ffp-contract=off, like ow_sky_light.hip and ow_solid_cast.hip.
//
//   k_mirror_apply  one lane per pixel, one 64-lane wave per 8 x 8 tile, as k_mist_apply: the mirror rays of a tile leave neighbouring
//                   points in neighbouring directions, so they pass the same few spheres.  A lane runs the sky pass up to radiance
//                   (mirror_begin), the wave searches the instances, and the lane finishes its record (mirror_finish).  The search:
//                     1. the box of the tile's ray origins and directions (twelve wave reductions, mirror_bundle_*);
//                     2. the instance spheres 64 at a time, one a lane, against that box (mirror_bundle_pass): a ballot of the few that
//                        any ray of the tile can pass at all -- 4 096 instances are 64 such rounds, not 4 096 sphere tests a lane;
//                     3. per survivor, read at a wave-uniform address, each lane's own solid_cast_sphere_pass; the lanes that pass are
//                        compacted by their ballot and all 64 lanes take the (pixel, triangle) items flat (the k-th pixel is the k-th
//                        set bit, as k_solid_cast takes its survivors), reading the pixel's ray from LDS (1.5 KB); a hit is a 64-bit
//                        LDS atomic min into the pixel's word (512 bytes).  Hits are rare, so the atomics are.
//                   The winner is a min over words, so the records, the hits and the counters do not depend on any of this: the CPU
//                   build walks every instance and every triangle on each lane in turn (mirror_search_lane) and gives the same bytes.
//                   Without the tile's box, and with each lane that passed walking the triangles itself, the pass took 3.3 and 4.7 times as long
//                   (profiles/EXPERIMENTS.md).  The five counters are summed across the wave with lane reads; lane 0 adds them to the
//                   block's copy (kMirrorSlots copies, a line each).  No scratch memory; nothing allocates.
#include <hip/hip_runtime.h>

#include "ow_kernels.h"

namespace ow {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
    return v;
}

__device__ __forceinline__ float wave_min(float v) {
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

__global__ void __launch_bounds__(64) k_mirror_apply(CameraParams cam, SkyLightParams lp, MirrorParams mp, SolidCastShape shape, SolidInstances in,
                                                     const SolidCastBound *bounds, int tiles_x, RenderPixel *pixels, SolidHit *hits,
                                                     unsigned long long *counters) {
    __shared__ float ray_o[3][64], ray_d[3][64];
    __shared__ unsigned long long best[64];
    const int lane = (int)threadIdx.x;
    const int tx = (int)blockIdx.x % tiles_x, ty = (int)blockIdx.x / tiles_x;
    const int i = 8 * tx + (lane & 7), j = 8 * ty + (lane >> 3);
    const bool inside = i < cam.width && j < cam.height;
    const size_t at = inside ? (size_t)j * cam.width + i : 0;
    char *rec = (char *)(pixels + at);
    MirrorPixel px;
    px.stage = kSkyLightLeft;
    px.cast = false;
    px.s.valid = false;
    u32x4 tail = {0u, 0u, 0u, 0u};
    float color[3] = {0.0f, 0.0f, 0.0f};
    if (inside) {
        const u32x4 head = *(const u32x4 *)rec;  // t, status, position.x, position.y
        const int32_t status = (int32_t)head.y;
        if (lp.camera_ok && (status & kRayHit) && !(status & (kRayEnvironment | kRaySkyLit))) {
            const u32x4 q1 = *(const u32x4 *)(rec + 16);  // position.z, p, wave_height
            const u32x4 q3 = *(const u32x4 *)(rec + 48);  // foam_factor, albedo
            const u32x4 q4 = *(const u32x4 *)(rec + 64);  // normal, fresnel
            const uint32_t rough = *(const uint32_t *)(rec + offsetof(RenderPixel, roughness));
            tail = *(const u32x4 *)(rec + offsetof(RenderPixel, specular));  // specular, color
            const float position[3] = {__uint_as_float(head.z), __uint_as_float(head.w), __uint_as_float(q1.x)};
            const float albedo[3] = {__uint_as_float(q3.y), __uint_as_float(q3.z), __uint_as_float(q3.w)};
            const float normal[3] = {__uint_as_float(q4.x), __uint_as_float(q4.y), __uint_as_float(q4.z)};
            color[0] = __uint_as_float(tail.y);
            color[1] = __uint_as_float(tail.z);
            color[2] = __uint_as_float(tail.w);
            mirror_begin(lp, mp, in.count, cam, i, j, status, position, albedo, normal, __uint_as_float(rough), color, px);
        }
    }
    const bool searching = px.cast && px.s.valid;
    const float T = mp.max_distance;
    uint32_t n_passed = 0u, n_pairs = 0u;
    uint64_t word = kSolidCastNoHit;
    if (__ballot(searching)) {
        MirrorBundle B;
        mirror_bundle_empty(B);
        if (searching) mirror_bundle_add(B, px.s);
        for (int k = 0; k < 3; ++k) {
            B.omin[k] = wave_min(B.omin[k]);
            B.omax[k] = wave_max(B.omax[k]);
            B.dmin[k] = wave_min(B.dmin[k]);
            B.dmax[k] = wave_max(B.dmax[k]);
            ray_o[k][lane] = px.s.o[k];
            ray_d[k][lane] = px.s.d[k];
        }
        mirror_bundle_close(B, T);
        best[lane] = kSolidCastNoHit;
        __syncthreads();
        const int nt = shape.num_triangles;
        for (int base = 0; base < in.count; base += 64) {
            bool candidate = false;
            if (base + lane < in.count) {
                const SolidCastBound b = bounds[base + lane];
                candidate = mp.cp.cull ? mirror_bundle_pass(B, b) : !(b.r < 0.0f);
            }
            for (uint64_t left = __ballot(candidate); left; left &= left - 1) {
                const int inst = base + __builtin_ctzll(left);  // wave-uniform
                const bool pass = searching && (!mp.cp.cull || solid_cast_sphere_pass(bounds[inst], px.s, T));
                const uint64_t m = __ballot(pass);
                if (!m) continue;
                if (pass) {
                    ++n_passed;
                    n_pairs += (uint32_t)nt;
                }
                const float *tf = solid_transform(in, inst);
                const int work = bit_count(m) * nt;  // <= 64 * 65536
                for (int f = lane; f < work; f += 64) {
                    const int k = f / nt, tri = f - k * nt;
                    const int src = solid_cast_select(m, k);
                    RaySetup rs;
                    rs.valid = true;
                    for (int c = 0; c < 3; ++c) {
                        rs.o[c] = ray_o[c][src];
                        rs.d[c] = ray_d[c][src];
                    }
                    const SolidCastPair pr = solid_cast_pair(shape, tf, rs, T, mp.cp.two_sided, tri);
                    if (pr.hit) atomicMin(&best[src], (unsigned long long)solid_cast_word(pr.t, inst * nt + tri));
                }
            }
        }
        __syncthreads();
        word = best[lane];
    }
    uint32_t n_pixels = 0u, n_rays = px.cast ? 1u : 0u, n_hits = 0u;
    if (inside) {
        SolidHit h = solid_hit_zero();
        h.instance = h.triangle = -1;
        if (px.cast) h = mirror_hit_record(shape, in, mp, px, word);
        if (px.stage != kSkyLightLeft) {
            mirror_finish(lp, mp, color, h, px);
            tail.y = __float_as_uint(px.sky.color[0]);
            tail.z = __float_as_uint(px.sky.color[1]);
            tail.w = __float_as_uint(px.sky.color[2]);
            *(u32x4 *)(rec + offsetof(RenderPixel, specular)) = tail;
            *(int32_t *)(rec + offsetof(RenderPixel, status)) = px.sky.status;
            n_pixels = 1u;
        }
        n_hits = (h.status & kRayHit) ? 1u : 0u;
        if (hits) {
            const u32x4 *src = (const u32x4 *)&h;
            u32x4 *dst = (u32x4 *)(hits + at);
            for (int k = 0; k < 4; ++k) dst[k] = src[k];
        }
    }
    n_pixels = wave_sum(n_pixels);  // at most 64, 64, 64 x 65536, 64 x 2^24 and 64
    n_rays = wave_sum(n_rays);
    n_passed = wave_sum(n_passed);
    n_pairs = wave_sum(n_pairs);
    n_hits = wave_sum(n_hits);
    if (lane == 0 && n_pixels) {
        unsigned long long *slot = counters + (size_t)(blockIdx.x % kMirrorSlots) * kMirrorSlotWords;
        atomicAdd(slot + kMirrorPixels, (unsigned long long)n_pixels);
        if (n_rays) atomicAdd(slot + kMirrorRays, (unsigned long long)n_rays);
        if (n_passed) atomicAdd(slot + kMirrorPassed, (unsigned long long)n_passed);
        if (n_pairs) atomicAdd(slot + kMirrorPairs, (unsigned long long)n_pairs);
        if (n_hits) atomicAdd(slot + kMirrorHits, (unsigned long long)n_hits);
    }
}

}  // namespace

hipError_t launch_mirror_apply(const MirrorArrays &A, const SolidInstances &in, const CameraParams &cam, const SkyLightParams &lp, const MirrorParams &mp,
                               RenderPixel *pixels_dev, SolidHit *hits_dev, hipStream_t s) {
    static_assert(offsetof(RenderPixel, position) == 8 && offsetof(RenderPixel, albedo) == 52 && offsetof(RenderPixel, normal) == 64 &&
                      offsetof(RenderPixel, roughness) == 80 && offsetof(RenderPixel, specular) == 96 && offsetof(RenderPixel, status) == 4 &&
                      sizeof(RenderPixel) == 128 && sizeof(SolidHit) == 64,
                  "the records' vectors");
    if (in.count > 0 && ((int64_t)in.count * A.shape.num_triangles > kSolidMaxProduct || in.count > kSolidMaxInstances)) return hipErrorInvalidValue;  // the host wrappers refuse these first
    if (hipError_t e = hipMemsetAsync(A.counters, 0, kMirrorCounterBytes, s); e != hipSuccess) return e;
    if (cam.width <= 0 || cam.height <= 0 || !pixels_dev) return hipSuccess;
    if (!lp.camera_ok && !hits_dev) return hipSuccess;  // a camera that is not finite changes nothing
    if (in.count > 0)
        if (hipError_t e = launch_solid_cast_bounds(in, A.shape_bound, A.bounds, (uint32_t *)A.counters, s); e != hipSuccess) return e;
    const SolidCastShape shape{A.shape.local, A.shape.indices, A.shape.num_vertices, A.shape.num_triangles};
    unsigned long long *sums = (unsigned long long *)((char *)A.counters + kMirrorSumsOffset);
    const int tiles_x = (cam.width + 7) / 8, tiles_y = (cam.height + 7) / 8;
    hipLaunchKernelGGL(k_mirror_apply, dim3(tiles_x * tiles_y), dim3(64), 0, s, cam, lp, mp, shape, in, A.bounds, tiles_x, pixels_dev, hits_dev, sums);
    return hipGetLastError();
}

}  // namespace ow

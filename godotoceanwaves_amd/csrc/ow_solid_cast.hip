// ow_solid_cast.hip -- the kernels of a ray cast against solids (ow_solid_cast.h holds the arithmetic, which tests/solid_cast/ also compiles
// as plain C++; the kernels are held to that build bit for bit).  Built with -ffp-contract=off, like ow_solid.hip.
//
//   k_solid_cast_shape_bound  one wave, once per shape (its first cast): the local centre and radius, kept in the ow_solid's block
//   k_solid_cast_bounds       one lane per instance, once per call: the instance's world sphere (radius < 0: skipped) into the context's
//                             scratch; the skipped instances are counted
//   k_solid_cast              one 64-lane wave per ray, 64-thread blocks, no LDS: the lanes stride over the instance spheres 64 at a time,
//                             the survivors of a round are compacted by their ballot (the k-th survivor is the k-th set bit), the lanes take
//                             the survivors' (instance, triangle) pairs flat, forming the three world vertices on the fly and keeping their
//                             smallest word; a 64-bit min across the wave (an xor tree of shuffles 32 .. 1); lane 0 rebuilds the winner's
//                             record and stores it as four 16-byte stores
//
// The counters of a call lie at the head of the scratch: the skipped instances, then kSolidCastSlots pairs of 64-bit sums (instances that
// passed the sphere test, pairs tested), one pair per 128 bytes; a wave adds into the slot of its block index, the host adds the slots up.
#include <hip/hip_runtime.h>

#include "ow_kernels.h"
#include "ow_solid_cast.h"

namespace ow {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

OW_DEV float wave_min(float v) {
    for (int d = 32; d >= 1; d >>= 1) {
        const float o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}
OW_DEV float wave_max(float v) {
    for (int d = 32; d >= 1; d >>= 1) {
        const float o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

__global__ void __launch_bounds__(64) k_solid_cast_shape_bound(const float *local, int num_vertices, SolidCastBound *out) {
    const int lane = (int)threadIdx.x;
    float lo[3], hi[3], c[3];
    solid_cast_box_lane(local, num_vertices, lane, lo, hi);
    for (int k = 0; k < 3; ++k) {
        lo[k] = wave_min(lo[k]);
        hi[k] = wave_max(hi[k]);
    }
    solid_cast_box_centre(lo, hi, c);
    const float d2 = wave_max(solid_cast_radius_lane(local, num_vertices, lane, c));
    if (lane == 0) *out = solid_cast_shape_sphere(c, d2);
}

__global__ void __launch_bounds__(256) k_solid_cast_bounds(SolidInstances in, const SolidCastBound *shape, SolidCastBound *out, uint32_t *skipped) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    bool skip = false;
    if (i < in.count) {
        const bool ok = solid_instance_ok(in, i);
        out[i] = solid_cast_instance_bound(solid_transform(in, i), ok, *shape);
        skip = !ok;
    }
    const uint64_t m = __ballot(skip);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(skipped, (uint32_t)__popcll(m));
}

// the 64 lanes of solid_cast_search, one each
struct DeviceWave {
    int lane;
    uint64_t best;
    template <class Pred>
    __device__ uint64_t ballot(const Pred &pred) {
        return __ballot(pred(lane));
    }
    template <class Fn>
    __device__ void lanes(const Fn &fn) {
        fn(lane, best);
    }
    __device__ uint64_t min_best() const {
        uint64_t v = best;
        for (int d = 32; d >= 1; d >>= 1) {
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
            const uint64_t o = ((uint64_t)hi << 32) | lo;
            v = o < v ? o : v;
        }
        return v;
    }
};

__global__ void __launch_bounds__(64) k_solid_cast(SolidCastShape shape, SolidInstances in, const SolidCastBound *bounds, SolidCastParams cp, const Ray *rays,
                                                   const RaycastHit *water, int count, unsigned long long *sums, SolidHit *out) {
    const int r = (int)blockIdx.x;
    if (r >= count) return;
    DeviceWave wave{(int)threadIdx.x, kSolidCastNoHit};
    const Ray ray = rays[r];
    float water_t = 0.0f;
    int32_t water_status = 0;
    if (water) {
        water_t = water[r].t;
        water_status = water[r].status;
    }
    uint64_t passed, pairs;
    const SolidCastWinner win = solid_cast_search(wave, shape, in, bounds, cp, ray, water != nullptr, water_t, water_status, passed, pairs);
    if (threadIdx.x == 0) {
        const SolidHit h = solid_cast_finish(shape, in, cp, win);
        const u32x4 *src = (const u32x4 *)&h;
        u32x4 *dst = (u32x4 *)(out + r);
        for (int k = 0; k < 4; ++k) dst[k] = src[k];
        if (passed) {
            unsigned long long *slot = sums + (size_t)(blockIdx.x % kSolidCastSlots) * kSolidCastSlotWords;
            atomicAdd(slot, (unsigned long long)passed);
            atomicAdd(slot + 1, (unsigned long long)pairs);
        }
    }
}

}  // namespace

hipError_t launch_solid_cast_shape_bound(const SolidShape &shape, SolidCastBound *bound_dev, hipStream_t s) {
    hipLaunchKernelGGL(k_solid_cast_shape_bound, dim3(1), dim3(64), 0, s, shape.local, shape.num_vertices, bound_dev);
    return hipGetLastError();
}

hipError_t launch_solid_cast_bounds(const SolidInstances &in, const SolidCastBound *shape_bound, SolidCastBound *bounds_dev, uint32_t *skipped_dev, hipStream_t s) {
    hipLaunchKernelGGL(k_solid_cast_bounds, dim3((unsigned)((in.count + 255) / 256)), dim3(256), 0, s, in, shape_bound, bounds_dev, skipped_dev);
    return hipGetLastError();
}

hipError_t launch_solid_cast(const SolidCastArrays &A, const SolidInstances &in, const SolidCastParams &cp, const Ray *rays_dev, const RaycastHit *water_dev,
                             int count, SolidHit *out_dev, hipStream_t s) {
    static_assert(sizeof(SolidHit) == 64, "the record's four 16-byte vectors");
    if ((int64_t)in.count * A.shape.num_triangles > kSolidMaxProduct || in.count > kSolidMaxInstances) return hipErrorInvalidValue;  // the host wrappers refuse these first
    if (hipError_t e = hipMemsetAsync(A.counters, 0, kSolidCastCounterBytes, s); e != hipSuccess) return e;
    if (count <= 0) return hipSuccess;
    if (in.count > 0)
        if (hipError_t e = launch_solid_cast_bounds(in, A.shape_bound, A.bounds, (uint32_t *)A.counters, s); e != hipSuccess) return e;
    const SolidCastShape shape{A.shape.local, A.shape.indices, A.shape.num_vertices, A.shape.num_triangles};
    hipLaunchKernelGGL(k_solid_cast, dim3((unsigned)count), dim3(64), 0, s, shape, in, A.bounds, cp, rays_dev, water_dev, count,
                       (unsigned long long *)((char *)A.counters + kSolidCastSumsOffset), out_dev);
    return hipGetLastError();
}

}  // namespace ow

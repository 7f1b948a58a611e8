// ow_raster.h -- the wave-level code of the kernels that draw triangles: k_mesh_* (ow_mesh.hip), k_solid_* (ow_solid.hip) and the shadow
// cast's k_shadow_* (ow_shadow.hip).  Device code only.  The clear, the vertex stage of an instanced draw, the walk over a triangle's box
// and (see count_classes for who calls it) the per-wave class count are here once; what differs between the pictures -- the set-up's type, the coverage rule, the word that is
// written -- is a target the walk is given.  The visibility-buffer target of the mesh and solid draws is below (its coverage rule is
// ow_mesh.h's tri_cover); the depth-map target is beside its kernel in ow_shadow.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "ow_solid.h"

namespace ow {

// the record lane `src` holds, src wave-uniform: one v_readlane_b32 per 32-bit word that is read afterwards, no LDS crossbar
template <typename T>
__device__ __forceinline__ T lane_read(const T &v, int src) {
    struct Ints {
        int w[sizeof(T) / 4];
    };
    static_assert(sizeof(T) % 4 == 0, "whole 32-bit words");
    Ints in = __builtin_bit_cast(Ints, v), out;
    for (int k = 0; k < (int)(sizeof(T) / 4); ++k) out.w[k] = __builtin_amdgcn_readlane(in.w[k], src);
    return __builtin_bit_cast(T, out);
}

// a clear kernel's body, one lane per word: `count` words to `value`, the four counters to zero
template <typename Word>
__device__ __forceinline__ void clear_words(Word *words, size_t count, Word value, uint32_t *counters) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) words[i] = value;
    if (i < 4) counters[i] = 0u;
}

// The classes of a wave's 64 set-ups, counted per wave and added once: `counter` is the counter this lane's set-up falls under (anything
// outside [first, last]: none).  k_shadow_raster counts through this; k_mesh_raster and k_solid_raster keep the same loop in their bodies,
// because with the call the compiler lays their sweep out differently and both draws measured 2.7 % slower
// (profiles/raster_shared_times.txt).
__device__ __forceinline__ void count_classes(uint32_t *counters, int lane, int counter, int first, int last) {
    for (int k = first; k <= last; ++k) {
        const uint64_t m = __ballot(counter == k);
        if (lane == 0 && m) atomicAdd(counters + k, (uint32_t)__popcll(m));
    }
}

// The vertex stage of an instanced draw, one lane per (instance, vertex) (instances * vertices <= 2^24): ow_solid.h's front end, then
// `vertex(transform, instance_ok, local)` makes the record, stored as 16-byte vectors.  Vertex 0's lane counts a skipped instance in
// *skipped.
template <typename Record, typename MakeVertex>
__device__ __forceinline__ void instance_vertices(const float *local, int num_vertices, const SolidInstances &in, Record *out, uint32_t *skipped,
                                                  MakeVertex vertex) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= in.count * num_vertices) return;
    const SolidSplit at = solid_split(i, num_vertices);
    const bool ok = solid_instance_ok(in, at.instance);
    if (!ok && at.item == 0) atomicAdd(skipped, 1u);
    const float l[3] = {local[3 * (size_t)at.item], local[3 * (size_t)at.item + 1], local[3 * (size_t)at.item + 2]};
    store_record(out + i, vertex(solid_transform(in, at.instance), ok, l));
}

// What one 64-lane wave does with the 64 set-ups its lanes hold (a class that is not drawn: nothing to do).  A lane whose box is at most
// lane_box centres a side walks it alone; the triangles with larger boxes are found by a ballot and taken one after the other by the whole
// wave, their set-up read from the owning lane (the source lane is wave-uniform: lane reads, no LDS), the 64 lanes sweeping the box in
// 8 x 8 tiles.  `id` is what this lane's set-up is known by in the picture (a triangle's index, a pair's number), lane `src`'s is
// id_base + src.  The target supplies:
//   Setup                       the set-up's type: 32-bit words only, with the box x0 .. x1, y0 .. y1 of the centres that may be covered
//   kLane, kWave                the values of Setup::kind for the two drawn classes
//   centre(s, i, j, id)         the coverage rule at centre (i, j) and the write where it is covered
template <typename Target>
__device__ __forceinline__ void raster_wave(const Target &target, const typename Target::Setup &s, int lane, int id, int id_base) {
    if (s.kind == Target::kLane) {
        for (int j = s.y0; j <= s.y1; ++j)
            for (int i = s.x0; i <= s.x1; ++i) target.centre(s, i, j, id);
    }
    uint64_t big = __ballot(s.kind == Target::kWave);
    while (big) {
        const int src = __builtin_ctzll(big);
        big &= big - 1;
        const typename Target::Setup o = lane_read(s, src);
        for (int ty = o.y0 >> 3; ty <= o.y1 >> 3; ++ty)
            for (int tx = o.x0 >> 3; tx <= o.x1 >> 3; ++tx) {
                const int i = 8 * tx + (lane & 7), j = 8 * ty + (lane >> 3);
                if (i < o.x0 || i > o.x1 || j < o.y0 || j > o.y1) continue;  // the box lies inside the picture: so does (i, j)
                target.centre(o, i, j, id_base + src);
            }
    }
}

__device__ __forceinline__ void vis_min(uint64_t *vis, size_t at, uint64_t word) {
    // the word only ever decreases: a stale read is at worst larger than what is there, and then the atomic is merely not spared
    if (word < vis[at]) atomicMin((unsigned long long *)(vis + at), (unsigned long long)word);
}

// The visibility buffer of k_mesh_raster and k_solid_raster as the walk's target: TriSetup's classes (its 13 plane words and its box
// are what the wave reads from the owning lane), tri_cover at a pixel centre, and (depth bits, id) written with a min.
struct VisTarget {
    typedef TriSetup Setup;
    const CameraParams &cam;
    const MeshParams &mp;
    uint64_t *vis;
    static constexpr int kLane = kTriLane, kWave = kTriWave;
    __device__ __forceinline__ void centre(const TriSetup &s, int i, int j, int id) const {
        const TriCover c = tri_cover(s.p, cam, mp.near, i, j);
        if (c.hit) vis_min(vis, (size_t)j * cam.width + i, mesh_word(c.depth, id));
    }
};

}  // namespace ow

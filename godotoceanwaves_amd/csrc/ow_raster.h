// ow_raster.h -- the wave-level half of the visibility-buffer rasteriser, shared by the kernels that draw triangles (k_mesh_raster in
// ow_mesh.hip, k_solid_raster in ow_solid.hip).  Device code only.  The coverage rule itself is ow_mesh.h's tri_cover.
#pragma once
#include <hip/hip_runtime.h>

#include "ow_mesh.h"

namespace ow {

__device__ __forceinline__ void vis_min(uint64_t *vis, size_t at, uint64_t word) {
    // the word only ever decreases: a stale read is at worst larger than what is there, and then the atomic is merely not spared
    if (word < vis[at]) atomicMin((unsigned long long *)(vis + at), (unsigned long long)word);
}

// the value lane `src` holds, src wave-uniform: one v_readlane_b32, no LDS crossbar
__device__ __forceinline__ int lane_read(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ float lane_read(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }

// What one 64-lane wave does with the 64 set-ups its lanes hold (s.kind < 0 or a culled class: nothing to draw).  A lane whose box is at most
// lane_box centres a side walks it alone; the triangles with larger boxes are found by a ballot and taken one after the other by the whole
// wave, their planes and box read from the owning lane (the source lane is wave-uniform: a lane read, no LDS), the 64 lanes sweeping the
// box in 8 x 8 tiles.  `id` is the low half of this lane's visibility words (a triangle's index, a pair's number), lane `src`'s is
// id_base + src.
__device__ __forceinline__ void raster_wave(const TriSetup &s, int lane, int id, int id_base, const CameraParams &cam, const MeshParams &mp, uint64_t *vis) {
    if (s.kind == kTriLane) {
        for (int j = s.y0; j <= s.y1; ++j)
            for (int i = s.x0; i <= s.x1; ++i) {
                const TriCover c = tri_cover(s.p, cam, mp.near, i, j);
                if (c.hit) vis_min(vis, (size_t)j * cam.width + i, mesh_word(c.depth, id));
            }
    }
    uint64_t big = __ballot(s.kind == kTriWave);
    while (big) {
        const int src = __builtin_ctzll(big);
        big &= big - 1;
        TriPlanes p;
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) p.n[a][b] = lane_read(s.p.n[a][b], src);
        for (int b = 0; b < 3; ++b) p.N[b] = lane_read(s.p.N[b], src);
        p.det = lane_read(s.p.det, src);
        const int x0 = lane_read(s.x0, src), x1 = lane_read(s.x1, src), y0 = lane_read(s.y0, src), y1 = lane_read(s.y1, src);
        const int t = id_base + src;
        for (int ty = y0 >> 3; ty <= y1 >> 3; ++ty)
            for (int tx = x0 >> 3; tx <= x1 >> 3; ++tx) {
                const int i = 8 * tx + (lane & 7), j = 8 * ty + (lane >> 3);
                if (i < x0 || i > x1 || j < y0 || j > y1) continue;
                const TriCover c = tri_cover(p, cam, mp.near, i, j);
                if (c.hit) vis_min(vis, (size_t)j * cam.width + i, mesh_word(c.depth, t));
            }
    }
}

}  // namespace ow

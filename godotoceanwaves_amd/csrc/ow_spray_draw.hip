// ow_spray_draw.hip -- the two kernels of a billboard draw (ow_spray_draw.h holds the arithmetic, which tests/spray_draw/ also compiles as
// plain C++; the kernels are held to that build bit for bit).  Built with -ffp-contract=off, like ow_spray.hip.
//
//   k_billboard_setup  one lane per slot of the draw list, 256 lanes per block; lanes at or beyond the device's live count have nothing to
//                      do.  :20-21 for the slot's instance -> a 32-byte sprite record (two 16-byte vector stores), and the slot's bit set
//                      with a 64-bit atomicOr in the mask of every coarse bin (bin_side x bin_side pixels) its pixel box touches.  Or-ing
//                      bits does not depend on the order.  Each wave ballots its drawn and culled lanes and adds them once.
//   k_billboard_blend  one 64-lane wave per 8 x 8 pixel tile, one lane per pixel (partial tiles at the right and bottom edges are masked).
//                      A lane loads 40 of its record's 128 bytes (t, status; specular, color; reserved), the wave walks its bin's mask 64
//                      words per trip, one word per lane: the words that are not zero are taken in ascending order (a ballot, then lane
//                      reads); within a word lane l tests bit l and, if set, that sprite's box against the tile (a second ballot); for each
//                      surviving bit in ascending order every lane evaluates that sprite for its own pixel and blends -- the sprite's address
//                      is wave-uniform.  Then color, the two reserved words and the RGBA8 word go out as vector stores.
//
// Slots ascend with the draw list, bits are taken in ascending order, and a pixel belongs to one lane: its fragments are blended in draw
// order whatever the scheduling.  The masks (bins x ceil(slots / 64) words) and the two counters are cleared per draw; no LDS, no sort,
// no device-side allocation.
#include <hip/hip_runtime.h>

#include "ow_kernels.h"

namespace ow {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

__global__ void __launch_bounds__(kBillboardSetupBlock) k_billboard_setup(const SprayInstance *instances, const uint32_t *draw_list, const uint32_t *live_count,
                                                                          uint32_t slots, CameraParams cam, SprayDrawParams dp, BillboardBins bins,
                                                                          SpraySprite *sprites, unsigned long long *masks, uint32_t *counters) {
    const uint32_t slot = blockIdx.x * kBillboardSetupBlock + threadIdx.x;
    uint32_t live = slots;
    if (live_count) live = min(*live_count, slots);
    bool listed = slot < live, drawn = false;
    if (listed) {
        const uint32_t index = draw_list ? draw_list[slot] : slot;
        listed = index < slots;  // always: the list holds indices below the emitter's amount
        if (listed) {
            struct InstanceWords {
                u32x4 v[sizeof(SprayInstance) / 16];
            };
            InstanceWords iw;
            const u32x4 *ip = (const u32x4 *)(instances + index);
            for (int k = 0; k < (int)(sizeof(SprayInstance) / 16); ++k) iw.v[k] = ip[k];
            const SprayInstance in = __builtin_bit_cast(SprayInstance, iw);
            SpraySprite sp;
            const bool ok = spray_sprite_setup(in, cam, dp, index, sp);
            struct SpriteWords {
                u32x4 v[2];
            };
            const SpriteWords sw = __builtin_bit_cast(SpriteWords, sp);
            u32x4 *dst = (u32x4 *)(sprites + slot);
            dst[0] = sw.v[0];
            dst[1] = sw.v[1];
            if (ok) {
                const SprayBox b = spray_sprite_box(sp, cam);
                if (!spray_box_empty(b)) {
                    drawn = true;
                    const unsigned long long bit = 1ull << (slot & 63u);
                    const size_t word = slot >> 6;
                    for (int by = b.y0 / bins.side; by <= b.y1 / bins.side; ++by)
                        for (int bx = b.x0 / bins.side; bx <= b.x1 / bins.side; ++bx)
                            atomicOr(masks + ((size_t)by * bins.nx + bx) * bins.words + word, bit);
                }
            }
        }
    }
    const uint64_t m_drawn = __ballot(drawn), m_culled = __ballot(listed && !drawn);
    if ((threadIdx.x & 63) == 0) {
        if (m_drawn) atomicAdd(counters + 0, (uint32_t)__popcll(m_drawn));
        if (m_culled) atomicAdd(counters + 1, (uint32_t)__popcll(m_culled));
    }
}

// the 64-bit value lane `src` holds, src wave-uniform: two lane reads, no LDS
__device__ __forceinline__ uint64_t lane_read64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

template <bool kRecords>
__global__ void __launch_bounds__(64) k_billboard_blend(CameraParams cam, SprayDrawParams dp, BillboardBins bins, const SpraySprite *sprites,
                                                        const unsigned long long *masks, int tiles_x, RenderPixel *pixels, uint32_t *rgba) {
    const int lane = (int)threadIdx.x;
    const int tx = (int)blockIdx.x % tiles_x, ty = (int)blockIdx.x / tiles_x;
    const int i = 8 * tx + (lane & 7), j = 8 * ty + (lane >> 3);
    const bool inside = i < cam.width && j < cam.height;
    const size_t at = inside ? (size_t)j * cam.width + i : 0;
    SprayPixel px;
    px.color[0] = dp.background[0];
    px.color[1] = dp.background[1];
    px.color[2] = dp.background[2];
    px.t = 0.0f;
    px.status = 0;
    px.count = px.last = 0u;
    u32x4 tail = u32x4{0u, 0u, 0u, 0u}, res = u32x4{0u, 0u, 0u, 0u};
    if (kRecords && inside) {
        const char *rec = (const char *)(pixels + at);
        const u32x2 head = *(const u32x2 *)rec;                                // t, status
        tail = *(const u32x4 *)(rec + offsetof(RenderPixel, specular));       // specular, color[3]
        res = *(const u32x4 *)(rec + offsetof(RenderPixel, reserved));
        px.t = __uint_as_float(head.x);
        px.status = (int32_t)head.y;
        px.color[0] = __uint_as_float(tail.y);
        px.color[1] = __uint_as_float(tail.z);
        px.color[2] = __uint_as_float(tail.w);
    }
    float x = 0.0f, y = 0.0f, rlen = 1.0f;
    if (inside) spray_pixel_ray(cam, i, j, x, y, rlen);
    // a tile lies in one bin: the bin's side is a multiple of 8
    const int x0 = 8 * tx, y0 = 8 * ty, x1 = min(x0 + 7, cam.width - 1), y1 = min(y0 + 7, cam.height - 1);
    const unsigned long long *mask = masks + ((size_t)(y0 / bins.side) * bins.nx + (x0 / bins.side)) * bins.words;
    for (int base = 0; base < bins.words; base += 64) {
        const uint64_t w = base + lane < bins.words ? mask[base + lane] : 0ull;
        uint64_t nz = __ballot(w != 0ull);
        while (nz) {
            const int src = __builtin_ctzll(nz);
            nz &= nz - 1;
            const uint64_t word = lane_read64(w, src);
            const size_t first = ((size_t)base + src) * 64;
            bool touch = false;
            if ((word >> lane) & 1ull) {
                const u32x4 *sp4 = (const u32x4 *)(sprites + first + lane);
                struct SpriteWords {
                    u32x4 v[2];
                };
                SpriteWords sw;
                sw.v[0] = sp4[0];
                sw.v[1] = sp4[1];
                const SprayBox b = spray_sprite_box(__builtin_bit_cast(SpraySprite, sw), cam);
                touch = b.x0 <= x1 && b.x1 >= x0 && b.y0 <= y1 && b.y1 >= y0;
            }
            uint64_t hits = __ballot(touch);
            while (hits) {
                const int bit = __builtin_ctzll(hits);
                hits &= hits - 1;
                const SpraySprite sp = sprites[first + bit];
                if (inside) spray_pixel_blend(sp, dp, x, y, rlen, px);
            }
        }
    }
    if (!inside) return;
    if (rgba) rgba[at] = pack_rgba8(px.color);
    if (kRecords) {
        char *rec = (char *)(pixels + at);
        tail.y = __float_as_uint(px.color[0]);
        tail.z = __float_as_uint(px.color[1]);
        tail.w = __float_as_uint(px.color[2]);
        res.y = px.count;
        res.z = px.last;
        *(u32x4 *)(rec + offsetof(RenderPixel, specular)) = tail;
        *(u32x4 *)(rec + offsetof(RenderPixel, reserved)) = res;
    }
}

}  // namespace

hipError_t launch_billboard_draw(const BillboardArrays &A, const CameraParams &cam, const SprayDrawParams &dp, const BillboardBins &bins, uint32_t *rgba_dev,
                                 RenderPixel *pixels_dev, hipStream_t s) {
    static_assert(offsetof(RenderPixel, specular) == 96 && offsetof(RenderPixel, reserved) == 112, "the record's last two 16-byte vectors");
    if (cam.width <= 0 || cam.height <= 0 || (!rgba_dev && !pixels_dev)) return hipSuccess;
    if (hipError_t e = hipMemsetAsync(A.counters, 0, A.clear_bytes, s); e != hipSuccess) return e;  // the counters and, behind them, the masks
    if (A.slots > 0) {
        const unsigned blocks = (A.slots + kBillboardSetupBlock - 1) / kBillboardSetupBlock;
        hipLaunchKernelGGL(k_billboard_setup, dim3(blocks), dim3(kBillboardSetupBlock), 0, s, A.instances, A.draw_list, A.live_count, A.slots, cam, dp, bins,
                           A.sprites, (unsigned long long *)A.masks, A.counters);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    const int tiles_x = (cam.width + 7) / 8, tiles_y = (cam.height + 7) / 8;
    if (pixels_dev)
        hipLaunchKernelGGL(k_billboard_blend<true>, dim3(tiles_x * tiles_y), dim3(64), 0, s, cam, dp, bins, A.sprites, (const unsigned long long *)A.masks,
                           tiles_x, pixels_dev, rgba_dev);
    else
        hipLaunchKernelGGL(k_billboard_blend<false>, dim3(tiles_x * tiles_y), dim3(64), 0, s, cam, dp, bins, A.sprites, (const unsigned long long *)A.masks,
                           tiles_x, pixels_dev, rgba_dev);
    return hipGetLastError();
}

}  // namespace ow

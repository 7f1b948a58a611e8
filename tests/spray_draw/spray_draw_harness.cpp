// spray_draw_harness.cpp -- godotoceanwaves_amd/csrc/ow_spray_draw.h compiled as plain C++ (g++ -ffp-contract=off): the CPU build of the
// billboard draw that tests/test_spray_draw.py holds to an FP64 twin written from the definition (tests/spray_draw_twin.py) and that the
// GPU kernels are held to bit for bit.  The draw here takes the kernels' route -- a sprite record per draw-list slot, one bit per slot in
// the mask of every coarse bin its pixel box touches, then 8 x 8 tiles that walk their bin's words in ascending order -- so that the bins, the
// boxes and the trips are the CPU build's too.  With -DSPRAY_DRAW_HARNESS_MAIN it is a stand-alone program that reads a case file (the
// header below, then the arrays), draws it and writes the picture: the form the sanitizers run.
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "ow_spray_draw.h"

using namespace ow;

extern "C" {

// one draw, every field four bytes: what the runtime resolves from its arguments (near <= 0 and bin_side 0 select the defaults here too)
struct CaseHeader {
    int32_t width, height;
    float cam[15];           // position, basis rows, tan(fov / 2), aspect, max_distance
    int32_t count;           // instances (an emitter's amount)
    int32_t live;            // entries of the draw list that count (has_list)
    int32_t has_list;        // 0: slot k draws instance k
    float time;
    float foam[3], max_alpha;
    int32_t aw, ah, asrgb, dw, dh, dsrgb;
    float near;
    float background[3];
    int32_t bin_side;
    int32_t has_pixels;
};

// sizeof and the offsets the Python side mirrors
void harness_billboard_sizes(int *out) {
    out[0] = (int)sizeof(BillboardMaterialOptions);
    out[1] = (int)sizeof(BillboardDrawOptions);
    out[2] = (int)offsetof(BillboardMaterialOptions, max_alpha);
    out[3] = (int)offsetof(BillboardMaterialOptions, albedo_srgb);
    out[4] = (int)offsetof(BillboardDrawOptions, background_color);
    out[5] = (int)offsetof(BillboardDrawOptions, bin_side);
    out[6] = (int)sizeof(SpraySprite);
    out[7] = (int)sizeof(CaseHeader);
}

void harness_srgb_table(float *out256) { spray_srgb_table(out256); }

}  // extern "C"

namespace {
CameraParams camera_of(const CaseHeader &h) {
    CameraParams cam;
    memcpy(cam.o, h.cam, 3 * sizeof(float));
    memcpy(cam.B, h.cam + 3, 9 * sizeof(float));
    cam.tan_half_fov = h.cam[12];
    cam.aspect = h.cam[13];
    cam.max_distance = h.cam[14];
    cam.width = h.width;
    cam.height = h.height;
    return cam;
}
SprayDrawParams params_of(const CaseHeader &h, const CameraParams &cam, const void *albedo, const void *dissolve, const float *table) {
    SprayDrawParams dp;
    for (int k = 0; k < 3; ++k) {
        dp.foam[k] = h.foam[k];
        dp.background[k] = h.background[k];
    }
    dp.max_alpha = h.max_alpha;
    dp.near = h.near > 0.0f ? h.near : kMeshDefaultNear;
    dp.time = h.time;
    dp.camera_ok = mesh_camera_ok(cam) ? 1 : 0;  // as the runtime evaluates it
    dp.albedo = SprayTexture{(const uint32_t *)albedo, h.aw, h.ah, h.asrgb};
    dp.dissolve = SprayTexture{(const uint32_t *)dissolve, h.dw, h.dh, h.dsrgb};
    dp.srgb = table;
    return dp;
}
}  // namespace

extern "C" {

// The draw.  pixels_inout: width x height records or null (background_color, no depth); rgba_out: width x height words or null;
// counters: billboards drawn and culled; bins_out: side, nx, ny, words as resolved.
void harness_billboard_draw(const CaseHeader *hp, const void *instances, const uint32_t *draw_list, const void *albedo, const void *dissolve,
                            void *pixels_inout, void *rgba_out, uint32_t *counters, int32_t *bins_out) {
    const CaseHeader &h = *hp;
    const CameraParams cam = camera_of(h);
    float table[256];
    spray_srgb_table(table);
    const SprayDrawParams dp = params_of(h, cam, albedo, dissolve, table);
    const uint32_t slots = (uint32_t)h.count;
    const BillboardBins bins = billboard_bins(h.width, h.height, slots, h.bin_side > 0 ? h.bin_side : kBillboardBinSide);
    if (bins_out) {
        bins_out[0] = bins.side;
        bins_out[1] = bins.nx;
        bins_out[2] = bins.ny;
        bins_out[3] = bins.words;
    }
    const SprayInstance *inst = (const SprayInstance *)instances;
    RenderPixel *pixels = h.has_pixels ? (RenderPixel *)pixels_inout : nullptr;
    uint32_t *rgba = (uint32_t *)rgba_out;
    // k_billboard_setup
    SpraySprite zero;
    memset(&zero, 0, sizeof(zero));
    std::vector<SpraySprite> sprites(slots ? slots : 1, zero);
    std::vector<uint64_t> masks((size_t)bins.nx * bins.ny * bins.words, 0);
    uint32_t drawn = 0, culled = 0;
    uint32_t live = slots;
    if (h.has_list) live = (uint32_t)h.live < slots ? (uint32_t)h.live : slots;
    for (uint32_t slot = 0; slot < live; ++slot) {
        const uint32_t index = h.has_list ? draw_list[slot] : slot;
        if (index >= slots) continue;
        SpraySprite sp;
        const bool ok = spray_sprite_setup(inst[index], cam, dp, index, sp);
        sprites[slot] = sp;
        bool is_drawn = false;
        if (ok) {
            const SprayBox b = spray_sprite_box(sp, cam);
            if (!spray_box_empty(b)) {
                is_drawn = true;
                for (int by = b.y0 / bins.side; by <= b.y1 / bins.side; ++by)
                    for (int bx = b.x0 / bins.side; bx <= b.x1 / bins.side; ++bx)
                        masks[((size_t)by * bins.nx + bx) * bins.words + (slot >> 6)] |= 1ull << (slot & 63u);
            }
        }
        drawn += is_drawn;
        culled += !is_drawn;
    }
    if (counters) {
        counters[0] = drawn;
        counters[1] = culled;
    }
    // k_billboard_blend
    const int tiles_x = (h.width + 7) / 8, tiles_y = (h.height + 7) / 8;
    for (int ty = 0; ty < tiles_y; ++ty)
        for (int tx = 0; tx < tiles_x; ++tx) {
            const int x0 = 8 * tx, y0 = 8 * ty, x1 = x0 + 7 < h.width - 1 ? x0 + 7 : h.width - 1, y1 = y0 + 7 < h.height - 1 ? y0 + 7 : h.height - 1;
            SprayPixel px[64];
            float x[64], y[64], rlen[64];
            for (int lane = 0; lane < 64; ++lane) {
                const int i = x0 + (lane & 7), j = y0 + (lane >> 3);
                SprayPixel &p = px[lane];
                for (int k = 0; k < 3; ++k) p.color[k] = dp.background[k];
                p.t = 0.0f;
                p.status = 0;
                p.count = p.last = 0u;
                x[lane] = y[lane] = 0.0f;
                rlen[lane] = 1.0f;
                if (i >= h.width || j >= h.height) continue;
                if (pixels) {
                    const RenderPixel &r = pixels[(size_t)j * h.width + i];
                    p.t = r.t;
                    p.status = r.status;
                    for (int k = 0; k < 3; ++k) p.color[k] = r.color[k];
                }
                spray_pixel_ray(cam, i, j, x[lane], y[lane], rlen[lane]);
            }
            const uint64_t *mask = masks.data() + ((size_t)(y0 / bins.side) * bins.nx + (x0 / bins.side)) * bins.words;
            for (int word = 0; word < bins.words; ++word) {
                uint64_t w = mask[word];
                while (w) {
                    const int bit = __builtin_ctzll(w);
                    w &= w - 1;
                    const SpraySprite &sp = sprites[(size_t)word * 64 + bit];
                    const SprayBox b = spray_sprite_box(sp, cam);
                    if (!(b.x0 <= x1 && b.x1 >= x0 && b.y0 <= y1 && b.y1 >= y0)) continue;
                    for (int lane = 0; lane < 64; ++lane) {
                        const int i = x0 + (lane & 7), j = y0 + (lane >> 3);
                        if (i < h.width && j < h.height) spray_pixel_blend(sp, dp, x[lane], y[lane], rlen[lane], px[lane]);
                    }
                }
            }
            for (int lane = 0; lane < 64; ++lane) {
                const int i = x0 + (lane & 7), j = y0 + (lane >> 3);
                if (i >= h.width || j >= h.height) continue;
                const size_t at = (size_t)j * h.width + i;
                if (rgba) rgba[at] = pack_rgba8(px[lane].color);
                if (pixels) {
                    for (int k = 0; k < 3; ++k) pixels[at].color[k] = px[lane].color[k];
                    pixels[at].reserved[1] = px[lane].count;
                    pixels[at].reserved[2] = px[lane].last;
                }
            }
        }
}

// One instance at one pixel, without a background: out = covered, passed, u, v, |VERTEX.xz|, depth_t, ALBEDO[3], ALPHA, then the sprite's
// C.x, C.y, s, hx, hy and whether the instance is drawn at all (16 floats)
void harness_billboard_fragment(const CaseHeader *hp, const void *instance, const void *albedo, const void *dissolve, int i, int j, float t,
                                int32_t status, float *out) {
    const CameraParams cam = camera_of(*hp);
    float table[256];
    spray_srgb_table(table);
    const SprayDrawParams dp = params_of(*hp, cam, albedo, dissolve, table);
    SpraySprite sp;
    const bool ok = spray_sprite_setup(*(const SprayInstance *)instance, cam, dp, 0u, sp);
    float x, y, rlen;
    spray_pixel_ray(cam, i, j, x, y, rlen);
    SprayFragment f;
    memset(&f, 0, sizeof(f));
    if (ok) f = spray_fragment(sp, dp, x, y, rlen, t, status);
    const float v[16] = {f.covered ? 1.0f : 0.0f, f.passed ? 1.0f : 0.0f, f.uv[0], f.uv[1], f.dist, f.depth_t, f.albedo[0], f.albedo[1], f.albedo[2],
                         f.alpha, sp.cx, sp.cy, sp.s, sp.hx, sp.hy, ok ? 1.0f : 0.0f};
    memcpy(out, v, sizeof(v));
}

}  // extern "C"

#ifdef SPRAY_DRAW_HARNESS_MAIN
namespace {
bool read_all(FILE *f, void *dst, size_t bytes) { return bytes == 0 || (dst && fread(dst, 1, bytes, f) == bytes); }
}  // namespace

// spray_draw_harness_main CASE OUT: reads the header and the arrays (instances, the draw list, the two textures, the records), draws, and
// writes the records (if any), the RGBA8 words and the two counters
int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s CASE OUT\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    CaseHeader h;
    if (!read_all(f, &h, sizeof(h)) || h.width < 1 || h.height < 1 || h.width > 8192 || h.height > 8192 || h.count < 0 || h.count > 1048576 || h.live < 0 ||
        h.live > h.count || h.aw < 1 || h.ah < 1 || h.dw < 1 || h.dh < 1 || h.aw > 4096 || h.ah > 4096 || h.dw > 4096 || h.dh > 4096) {
        fprintf(stderr, "bad case header\n");
        return 2;
    }
    const size_t count = (size_t)h.width * h.height;
    std::vector<SprayInstance> inst((size_t)h.count);
    std::vector<uint32_t> list(h.has_list ? (size_t)h.live : 0);
    std::vector<uint32_t> albedo((size_t)h.aw * h.ah), dissolve((size_t)h.dw * h.dh), rgba(count);
    std::vector<RenderPixel> pixels(h.has_pixels ? count : 0);
    if (!read_all(f, inst.data(), inst.size() * sizeof(SprayInstance)) || !read_all(f, list.data(), list.size() * 4) ||
        !read_all(f, albedo.data(), albedo.size() * 4) || !read_all(f, dissolve.data(), dissolve.size() * 4) ||
        !read_all(f, pixels.data(), pixels.size() * sizeof(RenderPixel))) {
        fprintf(stderr, "short case file\n");
        return 2;
    }
    fclose(f);
    uint32_t counters[2] = {0, 0};
    int32_t bins[4];
    harness_billboard_draw(&h, inst.data(), list.data(), albedo.data(), dissolve.data(), pixels.data(), rgba.data(), counters, bins);
    int bad = 0;
    for (const RenderPixel &p : pixels)
        for (int k = 0; k < 3; ++k) bad += !(fabsf(p.color[k]) <= 3.4028235e38f) && h.has_pixels;
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    if (!pixels.empty()) fwrite(pixels.data(), sizeof(RenderPixel), pixels.size(), o);
    fwrite(rgba.data(), 4, rgba.size(), o);
    fwrite(counters, 4, 2, o);
    fclose(o);
    printf("drawn=%u culled=%u bins=%dx%d side=%d words=%d not_finite=%d\n", counters[0], counters[1], bins[1], bins[2], bins[0], bins[3], bad);
    printf("ok\n");
    return 0;
}
#endif

// ow_spray_draw.h -- the sea-spray billboards drawn into a camera view (include/ocean_waves.h ow_billboard_*): sea_spray.gdshader's
// vertex() :18-24 and fragment() :26-34 over the instances of an emitter (ow_spray.h), blended in draw order over a picture of
// ow_mesh_draw or ow_render_view and depth-tested against it.
//
// Compiles as device code (ow_spray_draw.hip, built with -ffp-contract=off) and as plain C++ (tests/spray_draw/, g++ -ffp-contract=off),
// like ow_mesh.h: every FP32 operation is an IEEE-754 add, subtract, multiply, divide or square root, a floor, a conversion or a compare;
// exp is exp_f32 (ow_surface.h).  There is no library transcendental, so both builds produce the same bits for every input.
//
// WHAT THE SHADER TEXT DOES NOT CONTAIN, AS DECIDED HERE
//   billboard  The mesh is a QuadMesh of size 1 x 1 facing +Z (main.tscn's QuadMesh_06d3e).  :20 puts it at the instance's origin with the
//              camera's axes, :21 scales it by the lengths of the instance's basis columns.  In view space (x right, y up, z back) its
//              centre is C = B^T (origin - camera.position), mesh_vertex's operations in its order; its half extents are hx = |column 0| / 2
//              and hy = |column 1| / 2, |column k| = sqrtf((c0 c0 + c1 c1) + c2 c2) over rows 0, 1, 2.  The whole quad lies at view depth
//              s = -C.z.
//   coverage   Pixel (i, j)'s ray is (x, y, -1) with mesh_pixel_xy's x and y; it meets the quad's plane at (s x, s y, -s).  With
//              dx = s x - C.x and dy = s y - C.y the pixel is covered when |dx| <= hx, |dy| <= hy, hx > 0, hy > 0 and
//              near < s <= camera.max_distance.  Edges are inclusive, there is no anti-aliasing; a billboard behind the camera or before
//              the near plane covers nothing, and one depth means nothing is clipped.
//   varyings   UV = (dx / (2 hx) + 0.5, 0.5 - dy / (2 hy)): (0, 0) at the quad's top-left.  VERTEX.xz = (s x, -s).
//   fragment   :27-33 as written, products left to right: ALBEDO = (tex.rgb foam_color) (1.65, 1.75, 1.65);
//              distance_fade = 1 - exp_f32(-sqrtf((s x)(s x) + s s) 0.04); ALPHA = ((tex.a max_alpha) distance_fade)
//              max((custom.w + custom.z) 0.5 - dissolve.x, 0), the dissolve texture read at UV + TIME 0.35 (one FP32 product, one add per
//              axis).  The material is unshaded: the fragment's colour is ALBEDO.
//   texture()  Godot's sampler is engine code.  Here: level 0 only; repeat in both directions, taken first as u - floorf(u) (so the index
//              arithmetic is exact for every finite u); bilinear on texel centres, f = u W - 0.5, i0 = floorf(f), w = f - i0, the two indices
//              wrapped into [0, W); the four texels combined as bilinear() of ow_surface.h combines them:
//              (a (1 - wx) + b wx) (1 - wy) + (c (1 - wx) + d wx) wy.  A texel is RGBA8; R, G and B go through a 256-entry sRGB -> linear
//              table (spray_srgb_table: FP64 on the host, narrowed) unless the texture's flag turns it off (then byte / 255), A is a / 255.
//   depth      Against the background pixel's record: a fragment passes when the record has no kRayHit, or when its distance along the
//              pixel's normalised ray, s sqrtf((x x + y y) + 1) (mesh_pixel's form), is <= the record's t.  Spray writes no depth.
//   blend      dst = dst (1 - ALPHA) + ALBEDO ALPHA per channel (glsl_mix's form), in linear FP32; a channel whose result is not finite takes
//              ALBEDO.  Per pixel the fragments are blended in ascending order of the draw list (a MultiMesh draws its instances in that
//              order; the reference sets no depth sort).  A fragment whose ALPHA is not > 0 is not counted and changes nothing.
//   outputs    The record's color is replaced; reserved[1] is the number of fragments blended, reserved[2] the particle index + 1 of the
//              last one (0: none); the RGBA8 word is pack_rgba8's.  Every pixel of the image is written.
//   finite     An instance with a value that is not finite is skipped, and so is one whose C, hx, hy or (custom.w + custom.z) 0.5 is not
//              finite.  With a camera that is not finite (mesh_camera_ok) nothing is blended: every pixel keeps its colour.
#pragma once

#include <cmath>

#include "ow_mesh.h"
#include "ow_spray.h"

namespace ow {

// layout-identical to ow_billboard_material_options / ow_billboard_draw_options in include/ocean_waves.h
struct BillboardMaterialOptions {
    float foam_color[3], max_alpha;
    uint32_t albedo_srgb, dissolve_srgb;
    uint32_t reserved[10];
};
struct BillboardDrawOptions {
    float near;
    float background_color[3];
    int32_t bin_side;
    uint32_t flags;
    uint32_t reserved[10];
};
static_assert(sizeof(BillboardMaterialOptions) == 64 && sizeof(BillboardDrawOptions) == 64, "record layout");

constexpr int kBillboardTexMaxSide = 4096;     // OW_BILLBOARD_TEXTURE_MAX_SIDE
constexpr int kBillboardBinSide = 64;          // pixels a side of a coarse bin, by default
constexpr int kBillboardBinMax = 8192;         // ... and at most (one bin holds any image)
constexpr int kBillboardSetupBlock = 256;      // lanes per block of the set-up kernel
constexpr float kBillboardMaxAlpha = 0.666f;   // main.tscn:94

struct SprayTexture {
    const uint32_t *texels;  // [height][width] words R | G << 8 | B << 16 | A << 24 (the bytes R, G, B, A in memory)
    int width, height;
    int srgb;                // R, G, B through the table
};
// a draw's constants, resolved once from the material, the options and the clock
struct SprayDrawParams {
    float foam[3], max_alpha;
    float near;              // > 0
    float time;              // TIME
    float background[3];     // the colour of every pixel of a draw without records
    int camera_ok;           // 0: the camera is not finite -- nothing is blended
    SprayTexture albedo, dissolve;
    const float *srgb;       // [256] spray_srgb_table
};
// one billboard as the blend kernel reads it: 32 bytes
struct SpraySprite {
    float cx, cy, s;   // C.x, C.y, -C.z
    float hx, hy;
    float cz, cw;      // custom.z, custom.w
    uint32_t index;    // the particle's index
};
static_assert(sizeof(SpraySprite) == 32, "record layout");
struct SprayBox {
    int x0, x1, y0, y1;  // pixel centres that may be covered; empty when x0 > x1 or y0 > y1
};
// what the blend keeps of one pixel
struct SprayPixel {
    float color[3];
    float t;
    int32_t status;
    uint32_t count, last;
};

// the coarse bins of a draw: a billboard's slot sets one bit in the mask of every bin its pixel box touches
struct BillboardBins {
    int side;    // pixels a side of a bin, a multiple of 8 (an 8 x 8 tile lies in one bin)
    int nx, ny;  // bins across and down the image
    int words;   // 64-bit mask words per bin: ceil(slots / 64), at least 1
};
constexpr size_t kBillboardMaskCap = (size_t)64 << 20;  // bytes of masks a draw may hold: beyond it the bins' side doubles

// ---- the host's side (plain host C++ in both builds) -----------------------------------------------------------------------------------

// the bins of a width x height image and `slots` draw-list slots, from the side the options ask for
inline BillboardBins billboard_bins(int width, int height, uint32_t slots, int bin_side) {
    BillboardBins b;
    b.side = bin_side;
    b.words = (int)((slots + 63u) / 64u);
    if (b.words < 1) b.words = 1;
    for (;;) {
        b.nx = (width + b.side - 1) / b.side;
        b.ny = (height + b.side - 1) / b.side;
        if ((size_t)b.nx * b.ny * b.words * sizeof(uint64_t) <= kBillboardMaskCap || b.side >= kBillboardBinMax) break;
        b.side *= 2;
    }
    return b;
}

// IEC 61966-2-1 sRGB -> linear for the 256 byte values, in FP64, narrowed once
inline void spray_srgb_table(float out[256]) {
    for (int k = 0; k < 256; ++k) {
        const double c = (double)k / 255.0;
        out[k] = (float)(c <= 0.04045 ? c / 12.92 : std::pow((c + 0.055) / 1.055, 2.4));
    }
}

// ---- lane code ------------------------------------------------------------------------------------------------------------------------

// :20-21 for one instance: false where it is skipped (not finite, of zero extent, behind the near plane or beyond the far distance)
OW_DEV bool spray_sprite_setup(const SprayInstance &in, const CameraParams &cam, const SprayDrawParams &dp, uint32_t index, SpraySprite &sp) {
    sp.cx = sp.cy = sp.s = sp.hx = sp.hy = sp.cz = sp.cw = 0.0f;
    sp.index = index;
    if (!dp.camera_ok) return false;
    bool ok = true;
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 4; ++k) ok = ok && mesh_finite(in.row[r][k]);
    for (int k = 0; k < 4; ++k) ok = ok && mesh_finite(in.custom[k]);
    if (!ok) return false;
    float rel[3], C[3];
    for (int k = 0; k < 3; ++k) rel[k] = in.row[k][3] - cam.o[k];
    for (int k = 0; k < 3; ++k) C[k] = (cam.B[k] * rel[0] + cam.B[3 + k] * rel[1]) + cam.B[6 + k] * rel[2];  // column k of B
    const float hx = sqrtf((in.row[0][0] * in.row[0][0] + in.row[1][0] * in.row[1][0]) + in.row[2][0] * in.row[2][0]) * 0.5f;
    const float hy = sqrtf((in.row[0][1] * in.row[0][1] + in.row[1][1] * in.row[1][1]) + in.row[2][1] * in.row[2][1]) * 0.5f;
    const float s = -C[2];
    const float fade = (in.custom[3] + in.custom[2]) * 0.5f;
    ok = mesh_finite(C[0]) && mesh_finite(C[1]) && mesh_finite(C[2]) && mesh_finite(hx) && mesh_finite(hy) && mesh_finite(fade);
    if (!ok || !(hx > 0.0f) || !(hy > 0.0f) || !(s > dp.near) || !(s <= cam.max_distance)) return false;
    sp.cx = C[0];
    sp.cy = C[1];
    sp.s = s;
    sp.hx = hx;
    sp.hy = hy;
    sp.cz = in.custom[2];
    sp.cw = in.custom[3];
    return true;
}

// The box of pixel centres a billboard may cover: its rectangle projected (tri_setup's scale factors), widened by a sixteenth of a pixel for
// the projection's rounding and clamped to the image.  A bound that is not a number reads as the image's edge.
OW_DEV int spray_box_lo(float v, float hi) { return (int)ceilf(fminf(fmaxf(v, 0.0f), hi)); }     // a NaN reads as 0
OW_DEV int spray_box_hi(float v, float hi) { return (int)floorf(fmaxf(fminf(v, hi), -1.0f)); }   // a NaN reads as hi
OW_DEV SprayBox spray_sprite_box(const SpraySprite &sp, const CameraParams &cam) {
    const float W = (float)cam.width, H = (float)cam.height;
    const float sxp = W / (2.0f * cam.aspect * cam.tan_half_fov), syp = H / (2.0f * cam.tan_half_fov);
    const float lox = ((sp.cx - sp.hx) / sp.s) * sxp + 0.5f * W, hix = ((sp.cx + sp.hx) / sp.s) * sxp + 0.5f * W;
    const float loy = 0.5f * H - ((sp.cy + sp.hy) / sp.s) * syp, hiy = 0.5f * H - ((sp.cy - sp.hy) / sp.s) * syp;
    const float pad = 0.0625f;
    SprayBox b;
    b.x0 = spray_box_lo(lox - 0.5f - pad, W);
    b.x1 = spray_box_hi(hix - 0.5f + pad, W - 1.0f);
    b.y0 = spray_box_lo(loy - 0.5f - pad, H);
    b.y1 = spray_box_hi(hiy - 0.5f + pad, H - 1.0f);
    return b;
}
OW_DEV bool spray_box_empty(const SprayBox &b) { return b.x0 > b.x1 || b.y0 > b.y1; }

// one texel as four floats
OW_DEV void spray_texel(const SprayTexture &t, const float *srgb, int ix, int iy, float out[4]) {
    const uint32_t w = t.texels[(size_t)iy * t.width + ix];
    for (int k = 0; k < 3; ++k) {
        const uint32_t b = (w >> (8 * k)) & 0xffu;
        out[k] = t.srgb ? srgb[b] : (float)b / 255.0f;
    }
    out[3] = (float)(w >> 24) / 255.0f;
}
// the repeat and the two indices and the weight of one axis; u finite
OW_DEV void spray_tap(float u, int n, int &i0, int &i1, float &w) {
    const float r = u - floorf(u);                // [0, 1]: 1 where a tiny negative u rounds up
    const float f = r * (float)n - 0.5f;          // [-0.5, n - 0.5]
    const float f0 = floorf(f);
    w = f - f0;
    int i = (int)f0;                              // [-1, n - 1]
    if (i < 0) i += n;
    if (i >= n) i -= n;
    i0 = i;
    i1 = i + 1 == n ? 0 : i + 1;
}
OW_DEV void spray_texture(const SprayTexture &t, const float *srgb, float u, float v, float out[4]) {
    int x0, x1, y0, y1;
    float wx, wy;
    spray_tap(u, t.width, x0, x1, wx);
    spray_tap(v, t.height, y0, y1, wy);
    float a[4], b[4], c[4], d[4];
    spray_texel(t, srgb, x0, y0, a);
    spray_texel(t, srgb, x1, y0, b);
    spray_texel(t, srgb, x0, y1, c);
    spray_texel(t, srgb, x1, y1, d);
    const float ux = 1.0f - wx, uy = 1.0f - wy;
    for (int k = 0; k < 4; ++k) out[k] = (a[k] * ux + b[k] * wx) * uy + (c[k] * ux + d[k] * wx) * wy;
}

// what one billboard leaves at one pixel, for the records and the tests
struct SprayFragment {
    bool covered;   // the coverage rule
    bool passed;    // ... and the depth test
    float uv[2], dist, depth_t;
    float albedo[3], alpha;
};
// (x, y): mesh_pixel_xy's; rlen = sqrtf((x x + y y) + 1); t, status: the background record's
OW_DEV SprayFragment spray_fragment(const SpraySprite &sp, const SprayDrawParams &dp, float x, float y, float rlen, float t, int32_t status) {
    SprayFragment f;
    f.covered = f.passed = false;
    f.uv[0] = f.uv[1] = f.dist = f.depth_t = f.alpha = 0.0f;
    f.albedo[0] = f.albedo[1] = f.albedo[2] = 0.0f;
    const float px = sp.s * x, py = sp.s * y;
    const float dx = px - sp.cx, dy = py - sp.cy;
    if (!(fabsf(dx) <= sp.hx) || !(fabsf(dy) <= sp.hy)) return f;
    f.covered = true;
    f.depth_t = sp.s * rlen;
    if ((status & kRayHit) && !(f.depth_t <= t)) return f;
    f.passed = true;
    f.uv[0] = dx / (2.0f * sp.hx) + 0.5f;
    f.uv[1] = 0.5f - dy / (2.0f * sp.hy);
    float tex[4], dis[4];
    spray_texture(dp.albedo, dp.srgb, f.uv[0], f.uv[1], tex);
    const float k[3] = {1.65f, 1.75f, 1.65f};
    for (int c = 0; c < 3; ++c) f.albedo[c] = tex[c] * dp.foam[c] * k[c];                  // :28
    f.dist = sqrtf(px * px + sp.s * sp.s);
    const float distance_fade = 1.0f - exp_f32(-f.dist * 0.04f);                          // :30
    float alpha = tex[3] * dp.max_alpha;                                                  // :31
    alpha *= distance_fade;                                                               // :32
    const float shift = dp.time * 0.35f;
    spray_texture(dp.dissolve, dp.srgb, f.uv[0] + shift, f.uv[1] + shift, dis);
    alpha *= fmaxf((sp.cw + sp.cz) * 0.5f - dis[0], 0.0f);                                // :33
    f.alpha = alpha;
    return f;
}

// one billboard blended into one pixel
OW_DEV void spray_pixel_blend(const SpraySprite &sp, const SprayDrawParams &dp, float x, float y, float rlen, SprayPixel &px) {
    const SprayFragment f = spray_fragment(sp, dp, x, y, rlen, px.t, px.status);
    if (!f.passed || !(f.alpha > 0.0f)) return;
    for (int c = 0; c < 3; ++c) {
        const float v = px.color[c] * (1.0f - f.alpha) + f.albedo[c] * f.alpha;
        px.color[c] = mesh_finite(v) ? v : f.albedo[c];
    }
    px.count += 1u;
    px.last = sp.index + 1u;
}

// the ray of a pixel as the blend needs it
OW_DEV void spray_pixel_ray(const CameraParams &cam, int i, int j, float &x, float &y, float &rlen) {
    mesh_pixel_xy(cam, i, j, x, y);
    rlen = sqrtf((x * x + y * y) + 1.0f);
}

}  // namespace ow

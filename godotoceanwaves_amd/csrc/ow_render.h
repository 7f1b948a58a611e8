// ow_render.h -- camera views of the water (include/ocean_waves.h ow_render_view): per pixel, the ray through the pixel centre, the
// hit ow_raycast.h defines, water.gdshader's fragment() and light() at the hit (ow_shading.h) and a composite.
//
// Compiles as device code (ow_consumer.hip, built with -ffp-contract=off) and as plain C++ (tests/render/, g++ -ffp-contract=off), like
// ow_raycast.h: the same bits in both.  The device has no tangent: tan(fov / 2) and the aspect ratio are resolved by the host.
//
// Pixel (i, j), i along the row from the left, j down from the top, of a W x H image: the ray from the camera through the pixel centre,
//   direction = B * ((2 (i + 0.5) / W - 1) * aspect * th,  (1 - 2 (j + 0.5) / H) * th,  -1)        th = tan(fov_y / 2), aspect = W / H
// with B the camera's Godot Transform3D basis (rows; the camera looks down its -Z, +Y is up), normalised as ray_setup normalises it.
//
// The hit is ow_raycast.h's, step for step: the same slab, the same t_k, the same refinement points and the same final interpolation, so
// t, position, status and the query at the hit are the bits raycast_ray returns for that ray and the same RaycastParams.  raycast_ray's
// rule is "the first sample whose class differs from the first sample's", in the march and in each refinement round; one lane can
// therefore walk the samples in order and stop at the first change (march_pixel below) and reaches the bracket the 64-lane round
// finds.  It evaluates fewer samples than a round does (those past the change are never taken), which is why the samples / rounds
// counters of a ray-cast record are not part of a pixel.  Truncation falls on the same sample: the walk ends untruncated at the first k
// that is out of range, and truncated at k = max_samples if that k is still in range -- the two tests raycast_ray makes at the head of a
// round and after a partial one, in the same order.
//
// The composite is this library's choice (Godot's is engine code outside the reference): in linear FP32
//   color = ALBEDO * (DIFFUSE_LIGHT + ambient_color) + SPECULAR_LIGHT
// for a hit, from above or from below alike; sky_color for every pixel without one (a miss, a truncated march, an invalid ray).
// RGBA8 is (int)(clamp(c, 0, 1) * 255 + 0.5) per channel, alpha 255, no transfer curve; byte order R, G, B, A.
#pragma once

#include "ow_raycast.h"
#include "ow_shading.h"

namespace ow {

// layout-identical to ow_render_pixel in include/ocean_waves.h
struct RenderPixel {
    float t;
    int32_t status;
    float position[3];
    float p[2];
    float wave_height;
    float gradient_fragment[2];
    float foam_fragment;
    float dist;
    float foam_factor;
    float albedo[3];
    float normal[3];
    float fresnel;
    float roughness;
    float diffuse[3];
    float specular;
    float color[3];
    uint32_t reserved[4];
};
static_assert(sizeof(RenderPixel) == 128 && offsetof(RenderPixel, dist) == 44 && offsetof(RenderPixel, color) == 100, "record layout");

#if OW_DEVICE_BUILD
// A record whose size is a multiple of 16 bytes as 16-byte vectors, and its store to a 16-byte aligned address as that many vector stores:
// how every kernel writes a whole RenderPixel, MeshVertex or ShadowVertex.  (A kernel that touches chosen vectors only uses the type.)
template <typename T>
struct RecordWords {
    typedef uint32_t Vec __attribute__((ext_vector_type(4)));
    static_assert(sizeof(T) % 16 == 0, "whole 16-byte vectors");
    Vec v[sizeof(T) / 16];
};
template <typename T>
OW_DEV void store_record(T *dst, const T &rec) {
    const RecordWords<T> w = __builtin_bit_cast(RecordWords<T>, rec);
    for (int k = 0; k < (int)(sizeof(T) / 16); ++k) ((typename RecordWords<T>::Vec *)dst)[k] = w.v[k];
}
#endif

constexpr int kRenderMaxSide = 8192;  // OW_RENDER_MAX_SIDE

// the camera as the host resolves it from ow_camera
struct CameraParams {
    float o[3];          // position
    float B[9];          // basis rows: world = B * local
    float tan_half_fov;  // tan(fov_y / 2), FP64 on the host and narrowed
    float aspect;        // (float)W / (float)H
    float max_distance;
    int width, height;
};

OW_DEV Ray pixel_ray(const CameraParams &cam, int i, int j) {
    const float x = ((2.0f * ((float)i + 0.5f)) / (float)cam.width - 1.0f) * cam.aspect * cam.tan_half_fov;
    const float y = (1.0f - (2.0f * ((float)j + 0.5f)) / (float)cam.height) * cam.tan_half_fov;
    Ray r;
    for (int k = 0; k < 3; ++k) {
        r.origin[k] = cam.o[k];
        r.direction[k] = (cam.B[3 * k] * x + cam.B[3 * k + 1] * y) - cam.B[3 * k + 2];   // B * (x, y, -1)
    }
    r.max_distance = cam.max_distance;
    r.reserved = 0;
    return r;
}

// steps 2-3 of ow_raycast.h for one ray on one lane
struct PixelHit {
    float t;
    int32_t status;
    RaySetup s;
};
OW_DEV PixelHit march_pixel(const u16x4 *disp, int n, int cascades, const SurfaceScales &scales, const RaycastParams &rp, const Ray &ray,
                            float hw) {
    PixelHit out;
    out.t = 0.0f;
    out.s = ray_setup(ray, hw, rp.water_level);
    const RaySetup &s = out.s;
    if (!s.valid) {
        out.status = kRayInvalid;
        return out;
    }
    if (!s.enters) {
        out.status = s.below ? kRayFromBelow : 0;
        return out;
    }
    // 2. march: sample k, until its class differs from sample 0's
    bool above0 = false, bracket = false, truncated = false;
    float a = 0.0f, b = 0.0f, ga = 0.0f, gb = 0.0f;
    for (int k = 0;; ++k) {
        if (!march_in_range(s, rp.spacing, k)) break;  // the previous sample was t_out
        if (k >= rp.max_samples) {
            truncated = true;
            break;
        }
        const RaySample smp = ray_sample(disp, n, cascades, scales, rp, s, march_t(s, rp.spacing, k));
        const bool above = smp.g > 0.0f;
        if (k == 0) above0 = above;
        if (above != above0) {
            b = smp.t;
            gb = smp.g;
            bracket = true;
            break;
        }
        a = smp.t;
        ga = smp.g;
    }
    out.status = above0 ? 0 : kRayFromBelow;
    if (!bracket) {
        if (truncated) out.status |= kRayTruncated;
        return out;
    }
    // 3. refine: points j = 1 .. 63 of [a, b] in order, b itself as the 64th
    for (int i = 0; i < kRefineRounds && b - a > rp.tolerance; ++i) {
        const float ra = a, rb = b;
        for (int j = 1; j < 64; ++j) {
            const RaySample smp = ray_sample(disp, n, cascades, scales, rp, s, refine_t(ra, rb, j));
            if ((smp.g > 0.0f) != above0) {
                b = smp.t;
                gb = smp.g;
                break;
            }
            a = smp.t;
            ga = smp.g;
        }
    }
    const float w = ga / (ga - gb);
    float t = a + (b - a) * w;
    t = t > a ? (t < b ? t : b) : a;  // NaN -> a
    out.t = t;
    out.status |= kRayHit;
    return out;
}

OW_DEV uint32_t pack_rgba8(const float c[3]) {
    uint32_t w = 0xff000000u;
    for (int k = 0; k < 3; ++k) {
        const float v = c[k] > 0.0f ? (c[k] < 1.0f ? c[k] : 1.0f) : 0.0f;  // NaN -> 0
        w |= (uint32_t)(v * 255.0f + 0.5f) << (8 * k);
    }
    return w;
}

OW_DEV RenderPixel render_pixel_zero() {
    RenderPixel px;
    __builtin_memset(&px, 0, sizeof(px));
    return px;
}

// One pixel: the record (zeros, the status and sky_color in `color` without a hit) and its RGBA8 word.
OW_DEV RenderPixel render_pixel(const u16x4 *disp, const u16x4 *norm, int n, int cascades, const SurfaceScales &scales, const RaycastParams &rp,
                                const CameraParams &cam, const ShadeParams &sp, float hw, int i, int j, uint32_t *rgba) {
    RenderPixel px = render_pixel_zero();
    const Ray ray = pixel_ray(cam, i, j);
    const PixelHit hit = march_pixel(disp, n, cascades, scales, rp, ray, hw);
    px.status = hit.status;
    if (!(hit.status & kRayHit)) {
        for (int k = 0; k < 3; ++k) px.color[k] = sp.sky_color[k];
        *rgba = pack_rgba8(px.color);
        return px;
    }
    // 4. of ow_raycast.h: the position and the query there
    px.t = hit.t;
    for (int k = 0; k < 3; ++k) px.position[k] = hit.s.o[k] + hit.t * hit.s.d[k];
    const SurfaceQuery q = query_point(disp, norm, n, cascades, scales, rp.qp, px.position[0], px.position[2]);
    px.p[0] = q.p[0];
    px.p[1] = q.p[1];
    px.gradient_fragment[0] = q.sample.gradient_fragment[0];
    px.gradient_fragment[1] = q.sample.gradient_fragment[1];
    px.foam_fragment = q.sample.foam_fragment;
    // VIEW: the unit vector from the surface point to the camera; VERTEX.xz: the point along the camera's right (column 0 of B) and back
    // (column 2) axes.  A point that coincides with the camera has no direction: the ray's own -d^ stands in.
    float rel[3], view[3];
    for (int k = 0; k < 3; ++k) rel[k] = px.position[k] - cam.o[k];
    const float len = sqrtf(dot3(rel, rel));
    for (int k = 0; k < 3; ++k) view[k] = len > 0.0f ? -rel[k] / len : -hit.s.d[k];
    const float vx = (cam.B[0] * rel[0] + cam.B[3] * rel[1]) + cam.B[6] * rel[2];
    const float vz = (cam.B[2] * rel[0] + cam.B[5] * rel[1]) + cam.B[8] * rel[2];
    const Fragment f = shade_fragment(sp, q.sample, vx, vz, view);
    const Lighting l = shade_light(sp, f, view);
    px.wave_height = f.wave_height;
    px.dist = f.dist;
    px.foam_factor = f.foam_factor;
    px.fresnel = f.fresnel;
    px.roughness = f.roughness;
    px.specular = l.specular;
    for (int k = 0; k < 3; ++k) {
        px.albedo[k] = f.albedo[k];
        px.normal[k] = f.normal[k];
        px.diffuse[k] = l.diffuse[k];
        px.color[k] = f.albedo[k] * (l.diffuse[k] + sp.ambient_color[k]) + l.specular;
    }
    *rgba = pack_rgba8(px.color);
    return px;
}

}  // namespace ow

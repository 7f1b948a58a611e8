// ow_environment.h -- what finishes a camera picture (include/ocean_waves.h ow_sky_*, ow_environment_apply, ow_present): a panorama sky
// for the pixels nothing was drawn into, depth or exponential fog over the pixels something was, and the resolve / tonemap / transfer
// curve / adjustments / RGBA8 of the finished records.  The counterpart of main.tscn's Environment (:16-41) and Sun (:112-113).
//
// Compiles as device code (ow_environment.hip, built with -ffp-contract=off) and as plain C++ (tests/environment/, g++
// -ffp-contract=off), like ow_solid.h: every FP32 operation is an IEEE-754 add, subtract, multiply, divide or square root, a floor, a
// conversion or a compare; exp, log and pow are exp_f32 (ow_surface.h), log_f32 and pow_f32 (ow_shading.h); atan2 and acos are written
// out below.  There is no library transcendental, so both builds produce the same bits for every input.
//
// Everything here is THIS LIBRARY'S CHOICE modelled on Godot's renderer: the engine's source is not part of the reference, so this
// header is the authority for what the calls compute.
//
//   ray        pixel (i, j)'s ray is pixel_ray (ow_render.h), normalised as ray_setup normalises it: len = sqrtf((dx dx + dy dy) + dz dz),
//              d^ = d / len; a length that is 0 or not finite gives d^ = (0, 0, 0).
//   panorama   an equirectangular RGBA8 image, rows from the top.  For a unit direction d: u = atan2_f32(d.x, -d.z) / (2 pi) + 0.5,
//              v = acos_f32(d.y) / pi: -Z is the image's centre column, +Z its seam, +Y its top row.  Level 0 only, bilinear on texel
//              centres: along u ow_spray_draw.h's spray_tap (repeat), along v the same f = v H - 0.5, i0 = floorf(f), w = f - i0 with both
//              rows CLAMPED to [0, H - 1]; texels through spray_texel (R, G, B through spray_srgb_table unless the sky's flag turns it
//              off); the four combined as spray_texture combines them.  Alpha is not read.  sky(d) = texel(d) energy.  The engine reads
//              a blurred radiance level for aerial perspective; here the sky is always read unblurred.
//   sky fill   a pixel WITHOUT kRayHit: color = sky(d^); without a sky handle the colour is left as it is.  Not fogged (fog_sky_affect 0).
//   fog        a pixel WITH kRayHit, at d = record.t.
//              depth mode (fog_mode 1):  z = 0 where !(d > begin), 1 where d >= end, else smoothstep: q = (d - begin) / (end - begin),
//                                        z = (q q) (3 - 2 q); amount = clamp(pow_f32(z, curve) density, 0, 1)
//              exponential (fog_mode 0): a = -(d density); amount = clamp(a < 0 ? 1 - exp_f32(a) : 0, 0, 1)
//              fog colour: light_color; if aerial_perspective > 0, glsl_mix(light_color, S, aerial_perspective) per channel with
//              S = sky(d^), or sky_color without a sky handle; if sun_scatter > 0.001, plus (sun_color p) sun_scatter with
//              p = max(dot3(d^, sun^), 0)^8 as three squarings, sun^ normalised in FP64 by the host.
//              color = glsl_mix(color, fog colour, amount) per channel; a channel that is not finite takes the fog colour.
//   status     every pixel that is processed gets kRayEnvironment; a pixel that carries it already is left alone (applying twice is
//              applying once).  Nothing but color and status changes.  A camera that is not finite (mesh_camera_ok) changes nothing.
//   out of scope: height fog, volumetric fog, the FogVolume node (ow_mist.h's pass, which goes after this one); light FROM the sky on the surfaces (its irradiance, its blurred radiance
//              levels in the water) is ow_sky_light.h's pass, which goes before this one; this pass still reads the sky unblurred.  Spray drawn afterwards is not fogged: the emitter sits tens of metres
//              from the camera, where the scene's depth fog (from 200 m) is 0.
//
//   present    per OUTPUT pixel of a (W / s) x (H / s) image, s = downsample in 1 .. 4:
//     resolve  sum the s s records' color row-major in FP32 from 0, a channel that is not finite counting as 0; times the FP32 constant
//              1 / (s s); a result that is not finite (the sum overflowed) is 0.  linear_out = (r, g, b, hits / (s s)).
//     exposure c = c exposure
//     tonemap  c = min(max(c, 0), 1e18) (the cap keeps every mode finite; all are within 1e-17 of their limit there), then
//              0 linear    c
//              1 Reinhard  (w2 c + c c) / (w2 c + w2), w2 = white white
//              2 filmic    f(c) / f(white), f(x) = (x (A x + C B) + D E) / (x (A x + B) + D F) - (D E) / (D F), A 0.88, B 0.6, C 0.1,
//                          D 0.2, E 0.01, F 0.3: E / F is written as the first term's value at x = 0, so that f(0) is exactly 0
//     curve    with srgb: c = clamp(c, 0, 1); c < 0.0031308 ? 12.92 c : 1.055 pow_f32(c, 1 / 2.4) - 0.055
//     adjust   c = glsl_mix(0, c, brightness); c = glsl_mix(0.5, c, contrast); c = glsl_mix(((r + g) + b) 0.33333, c, saturation)
//     pack     pack_rgba8 (ow_render.h)
#pragma once

#include <cmath>

#include "ow_mesh.h"
#include "ow_render.h"
#include "ow_spray_draw.h"

namespace ow {

// layout-identical to ow_sky_options, ow_environment_options and ow_present_options in include/ocean_waves.h
struct SkyOptions {
    uint32_t srgb;
    float energy;
    uint32_t reserved[6];
};
struct EnvironmentOptions {
    int32_t fog_mode;
    float density;
    float depth_begin, depth_end, depth_curve;
    float aerial_perspective;
    float sun_scatter;
    uint32_t flags;
    float light_color[3];
    float sun_color[3];
    float sun_direction[3];
    float sky_color[3];
    uint32_t reserved[12];
};
struct PresentOptions {
    int32_t downsample;
    int32_t tonemap;
    float exposure, white;
    uint32_t srgb;
    float brightness, contrast, saturation;
    uint32_t flags;
    uint32_t reserved[7];
};
static_assert(sizeof(SkyOptions) == 32 && sizeof(EnvironmentOptions) == 128 && offsetof(EnvironmentOptions, light_color) == 32 &&
                  offsetof(EnvironmentOptions, reserved) == 80 && sizeof(PresentOptions) == 64 && offsetof(PresentOptions, reserved) == 36,
              "record layout");

constexpr int32_t kRayEnvironment = 32;         // OW_RAY_ENVIRONMENT
constexpr int kSkyMaxSide = 8192;               // OW_SKY_MAX_SIDE
constexpr int kPresentMaxDownsample = 4;        // OW_PRESENT_MAX_DOWNSAMPLE
constexpr int kFogExponential = 0, kFogDepth = 1;
constexpr int kTonemapLinear = 0, kTonemapReinhard = 1, kTonemapFilmic = 2;
constexpr float kEnvColorMax = 1.0e12f;         // the largest magnitude of a colour, the energy and the fog distances the options take
constexpr float kEnvCurveMin = 0.01f, kEnvCurveMax = 100.0f;
constexpr float kPresentWhiteMin = 0.01f, kPresentScaleMax = 1.0e6f;  // white in [0.01, 1e6], exposure in [0, 1e6]
constexpr float kPresentAdjustMax = 8.0f;       // brightness, contrast and saturation in [0, 8]
constexpr float kPresentCap = 1.0e18f;          // the tonemap's input is at most this

// an environment pass's constants, resolved once from the options and the sky
struct EnvParams {
    int camera_ok;  // 0: the camera is not finite -- nothing changes
    int fog_mode;
    float density, begin, end, curve, aerial, scatter;
    float light_color[3], sun_color[3], sun[3], sky_color[3];
    int has_sky;
    SprayTexture sky;
    const float *srgb;  // [256] spray_srgb_table
    float energy;
};
// a present's constants
struct PresentParams {
    int s;       // 1 .. 4
    float inv;   // 1 / (s s), FP32
    int tonemap;
    float exposure, white;
    int srgb;
    float brightness, contrast, saturation;
};

OW_DEV float env_clamp01(float v) { return v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f; }  // a NaN -> 0

// atan2(y, x) in the basic operations.  q = min(|x|, |y|) / max(|x|, |y|) in [0, 1]; above tan(pi / 8) it is reduced to (q - 1) / (q + 1)
// around pi / 4; the arctangent of the reduced argument (|z| <= 0.4143) is the classic single-precision odd polynomial of degree 9; then
// the octant: pi / 2 - r where |y| > |x|, pi - r where x < 0, negated where y < 0 -- each constant as a high and a low FP32 part.  A zero
// of either sign counts as +0 (so atan2_f32(0, x < 0) is +pi), atan2_f32(0, 0) is 0, and an argument that is not finite gives 0.
// Largest error against the FP64 library over a sweep of 2^20 directions round the circle at magnitudes from 1e-30 to 1e30 and as many on
// the unit circle, with the axes, the diagonals, the seam (x < 0, |y| from 1 down to 1e-30) and both poles (|y| down to 1e-30 against
// x = +-1): 2.54 ulp of the result (at y / x = -0.4148, just past the reduction's breakpoint; mean 0.33), 3.0e-7 absolute
// (tests/test_environment.py measures and asserts both, as tests/test_render_view.py does for log_f32).
// acos_f32(y) = atan2_f32(sqrtf(max((1 - y) (1 + y), 0)), y) in [0, pi]: within 3.2e-7 of the FP64 library's acos over [-1, 1], the poles
// included (1 - y is exact there, so nothing cancels).  The same bits on the device and on the host.
OW_DEV float atan2_f32(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    if (!(ax <= 3.4028235e38f) || !(ay <= 3.4028235e38f)) return 0.0f;
    const float mx = ax > ay ? ax : ay, mn = ax > ay ? ay : ax;
    if (!(mx > 0.0f)) return 0.0f;
    const float q = mn / mx;
    const bool upper = q > 0.414213562f;
    const float z = upper ? (q - 1.0f) / (q + 1.0f) : q;
    const float zz = z * z;
    float p = 8.05374449538e-2f;
    p = p * zz - 1.38776856032e-1f;
    p = p * zz + 1.99777106478e-1f;
    p = p * zz - 3.33329491539e-1f;
    float r = (p * zz) * z + z;
    if (upper) r = (r + -2.18556941e-8f) + 0.785398185f;       // + pi / 4
    if (ay > ax) r = (-4.37113883e-8f - r) + 1.57079637f;      // pi / 2 - r
    if (x < 0.0f) r = (-8.74227766e-8f - r) + 3.14159274f;     // pi - r
    return y < 0.0f ? -r : r;
}
OW_DEV float acos_f32(float y) {
    const float c = (1.0f - y) * (1.0f + y);  // 1 - y y without the cancellation at the poles: 1 - y is exact for y in [0.5, 2]
    return atan2_f32(sqrtf(c > 0.0f ? c : 0.0f), y);
}

// the unit direction of pixel (i, j); zeros where the ray has no direction
OW_DEV void env_ray(const CameraParams &cam, int i, int j, float d[3]) {
    const Ray r = pixel_ray(cam, i, j);
    bool ok = true;
    for (int k = 0; k < 3; ++k) ok = ok && mesh_finite(r.direction[k]);
    const float len = ok ? sqrtf((r.direction[0] * r.direction[0] + r.direction[1] * r.direction[1]) + r.direction[2] * r.direction[2]) : 0.0f;
    ok = ok && len > 0.0f && mesh_finite(len);
    for (int k = 0; k < 3; ++k) d[k] = ok ? r.direction[k] / len : 0.0f;
}

// where a unit direction falls in the panorama
OW_DEV void sky_uv(const float d[3], float &u, float &v) {
    u = atan2_f32(d[0], -d[2]) / 6.28318548f + 0.5f;
    v = acos_f32(d[1]) / 3.14159274f;
}
// the two rows and the weight along v: spray_tap's arithmetic with the rows clamped instead of wrapped; v in [0, 1]
OW_DEV void sky_tap_rows(float v, int n, int &i0, int &i1, float &w) {
    const float f = v * (float)n - 0.5f;  // [-0.5, n - 0.5]
    const float f0 = floorf(f);
    w = f - f0;
    const int i = (int)f0;                // [-1, n - 1]
    i0 = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
    i1 = i + 1 > n - 1 ? n - 1 : i + 1;
}
// the panorama along d, before the energy
OW_DEV void sky_texture(const SprayTexture &t, const float *srgb, const float d[3], float out[3]) {
    float u, v;
    sky_uv(d, u, v);
    int x0, x1, y0, y1;
    float wx, wy;
    spray_tap(u, t.width, x0, x1, wx);
    sky_tap_rows(v, t.height, y0, y1, wy);
    float a[4], b[4], c[4], e[4];
    spray_texel(t, srgb, x0, y0, a);
    spray_texel(t, srgb, x1, y0, b);
    spray_texel(t, srgb, x0, y1, c);
    spray_texel(t, srgb, x1, y1, e);
    const float ux = 1.0f - wx, uy = 1.0f - wy;
    for (int k = 0; k < 3; ++k) out[k] = (a[k] * ux + b[k] * wx) * uy + (c[k] * ux + e[k] * wx) * wy;
}

OW_DEV float fog_amount(const EnvParams &ep, float d) {
    if (ep.fog_mode == kFogDepth) {
        float z;
        if (!(d > ep.begin)) {
            z = 0.0f;
        } else if (d >= ep.end) {
            z = 1.0f;
        } else {
            const float q = (d - ep.begin) / (ep.end - ep.begin);
            z = (q * q) * (3.0f - 2.0f * q);
        }
        return env_clamp01(pow_f32(z, ep.curve) * ep.density);
    }
    const float a = -(d * ep.density);
    return env_clamp01(a < 0.0f ? 1.0f - exp_f32(a) : 0.0f);
}

// what the pass makes of one pixel, with the intermediates the tests read
struct EnvPixel {
    bool changed;       // color and status are to be written
    int32_t status;
    float color[3];
    float ray[3];
    float sky[3];       // sky(d^) (sky_color without a handle); zeros where it was not needed
    float amount;       // of fog; 0 for a pixel without a hit
    float fog[3];       // the fog colour; zeros for a pixel without a hit
};
OW_DEV EnvPixel environment_pixel(const EnvParams &ep, const CameraParams &cam, int i, int j, float t, int32_t status, const float color[3]) {
    EnvPixel px;
    px.changed = false;
    px.status = status;
    px.amount = 0.0f;
    for (int k = 0; k < 3; ++k) {
        px.color[k] = color[k];
        px.ray[k] = px.sky[k] = px.fog[k] = 0.0f;
    }
    if (!ep.camera_ok || (status & kRayEnvironment)) return px;
    px.changed = true;
    px.status = status | kRayEnvironment;
    env_ray(cam, i, j, px.ray);
    const bool hit = (status & kRayHit) != 0;
    if (hit ? ep.aerial > 0.0f : ep.has_sky != 0) {
        if (ep.has_sky) {
            sky_texture(ep.sky, ep.srgb, px.ray, px.sky);
            for (int k = 0; k < 3; ++k) px.sky[k] *= ep.energy;
        } else {
            for (int k = 0; k < 3; ++k) px.sky[k] = ep.sky_color[k];
        }
    }
    if (!hit) {
        if (ep.has_sky)
            for (int k = 0; k < 3; ++k) px.color[k] = px.sky[k];
        return px;
    }
    px.amount = fog_amount(ep, t);
    for (int k = 0; k < 3; ++k) px.fog[k] = ep.light_color[k];
    if (ep.aerial > 0.0f)
        for (int k = 0; k < 3; ++k) px.fog[k] = glsl_mix(px.fog[k], px.sky[k], ep.aerial);
    if (ep.scatter > 0.001f) {
        const float c = fmaxf(dot3(px.ray, ep.sun), 0.0f);
        const float c2 = c * c, c4 = c2 * c2, c8 = c4 * c4;
        for (int k = 0; k < 3; ++k) px.fog[k] += (ep.sun_color[k] * c8) * ep.scatter;
    }
    for (int k = 0; k < 3; ++k) {
        const float v = glsl_mix(color[k], px.fog[k], px.amount);
        px.color[k] = mesh_finite(v) ? v : px.fog[k];
    }
    return px;
}

// ---- present ---------------------------------------------------------------------------------------------------------------------------

OW_DEV float tonemap_filmic_f(float x) {
    const float A = 0.88f, B = 0.6f, C = 0.1f, D = 0.2f, E = 0.01f, F = 0.3f;
    return (x * (A * x + C * B) + D * E) / (x * (A * x + B) + D * F) - (D * E) / (D * F);
}
OW_DEV float present_tonemap(const PresentParams &pp, float c) {
    c = c > 0.0f ? (c < kPresentCap ? c : kPresentCap) : 0.0f;  // a NaN -> 0
    if (pp.tonemap == kTonemapReinhard) {
        const float w2 = pp.white * pp.white;
        return (w2 * c + c * c) / (w2 * c + w2);
    }
    if (pp.tonemap == kTonemapFilmic) return tonemap_filmic_f(c) / tonemap_filmic_f(pp.white);
    return c;
}
OW_DEV float present_srgb(float c) {
    c = env_clamp01(c);
    return c < 0.0031308f ? 12.92f * c : 1.055f * pow_f32(c, 0.416666667f) - 0.055f;
}
// the stages of one output pixel past the resolve, each kept for the tests
struct PresentStages {
    float exposed[3], mapped[3], encoded[3], adjusted[3];
};
OW_DEV uint32_t present_encode(const PresentParams &pp, const float lin[3], PresentStages &st) {
    for (int k = 0; k < 3; ++k) {
        st.exposed[k] = lin[k] * pp.exposure;
        st.mapped[k] = present_tonemap(pp, st.exposed[k]);
        st.encoded[k] = pp.srgb ? present_srgb(st.mapped[k]) : st.mapped[k];
    }
    float c[3];
    for (int k = 0; k < 3; ++k) {
        c[k] = glsl_mix(0.0f, st.encoded[k], pp.brightness);
        c[k] = glsl_mix(0.5f, c[k], pp.contrast);
    }
    const float grey = ((c[0] + c[1]) + c[2]) * 0.33333f;
    for (int k = 0; k < 3; ++k) st.adjusted[k] = glsl_mix(grey, c[k], pp.saturation);
    return pack_rgba8(st.adjusted);
}
// One output pixel from its s x s block of records (block: the top-left one; row_stride: records per row of the picture).  lin: the
// resolved linear colour and the share of the block's records with kRayHit.
OW_DEV uint32_t present_pixel(const PresentParams &pp, const RenderPixel *block, size_t row_stride, float lin[4], PresentStages &st) {
    float sum[3] = {0.0f, 0.0f, 0.0f};
    int hits = 0;
    for (int r = 0; r < pp.s; ++r)
        for (int c = 0; c < pp.s; ++c) {
            const RenderPixel *rec = block + (size_t)r * row_stride + c;
            for (int k = 0; k < 3; ++k) {
                const float v = rec->color[k];
                sum[k] += mesh_finite(v) ? v : 0.0f;
            }
            hits += (rec->status & kRayHit) ? 1 : 0;
        }
    for (int k = 0; k < 3; ++k) {
        const float v = sum[k] * pp.inv;
        lin[k] = mesh_finite(v) ? v : 0.0f;
    }
    lin[3] = (float)hits * pp.inv;
    return present_encode(pp, lin, st);
}

}  // namespace ow

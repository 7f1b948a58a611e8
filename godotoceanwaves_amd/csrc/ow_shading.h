// ow_shading.h -- the water shader's shading math at one surface point: water.gdshader fragment() lines 73-93 past the texture reads
// (which ow_surface.h's sample_point already holds as gradient_fragment / foam_fragment) and all of light(), lines 96-127, for one
// directional light.  What ow_render.h's per-pixel record is made of.
//
// Compiles as device code (ow_consumer.hip, built with -ffp-contract=off) and as plain C++ (tests/render/, g++ -ffp-contract=off), like
// ow_surface.h and ow_raycast.h: every operation is an IEEE-754 FP32 add, multiply, divide, square root, min / max or compare, or integer
// work on the exponent field, so both builds produce the same bits.  There is no library log() or pow(): the one power with a
// fractional exponent goes through log_f32 and exp_f32; every other pow() of the shader has a small integer exponent and is written as
// multiplications.  The two constants that depend on uniforms alone are computed by the host in FP64 and narrowed once.
//
// NORMAL stays in world space.  The shader rotates it into view space (line 90: VIEW_MATRIX * ...), but every later use is a dot
// product with VIEW or LIGHT, which a rotation leaves alone: here VIEW and LIGHT are world-space unit vectors instead.
//
// Guards, so that nothing returned is NaN or Inf where GLSL would give one (each is named again at its statement):
//   G1  a fresnel base 1 - dot(VIEW, NORMAL) that rounding made negative is clamped at 0 (GLSL: pow of a negative base, undefined)
//   G2  sqrt(1 - c c) of a c rounded above 1 takes 0 (GLSL: sqrt of a negative number)
//   G3  a masking term whose denominator is 0 (roughness 0) is kMaskCap instead of +Inf; so is any value above it
//   G4  the GGX term is 0 where GLSL has 0 / 0 (roughness 0, NORMAL = halfway) and at most kMaskCap
//   G5  halfway of LIGHT = -VIEW is the zero vector instead of normalize(0)
//   G6  log_f32 of 0, of a negative number or of a NaN is -3.4028235e38 (it is only called on a base > 0)
#pragma once

#include "ow_surface.h"

namespace ow {

// ln x in the basic operations: x = m 2^e with m in [sqrt(1/2), sqrt(2)) from the exponent field (a subnormal x is scaled by 2^23
// first); s = (m - 1) / (m + 1), |s| <= 0.1716; ln m = 2 s (1 + s^2/3 + s^4/5 + s^6/7 + s^8/9) (truncation below 3e-9 relative);
// ln x = e ln2_hi + (e ln2_lo + ln m) with exp_f32's Cody-Waite split, whose high part times e is exact.  Largest error against the
// FP64 library over a logarithmic sweep of (0, 4], the smallest normal, 1 -+ ulp and the exact powers of two: 1.94 ulp (at
// x = 1.03112; mean 0.28; tests/test_render_view.py measures and asserts it; exp_f32's is "a few ulp").  exp_f32 is written for
// a <= 0 but holds for the small positive arguments a back-facing fresnel base gives (a <= 5 ln 2).  The same bits on the device and
// on the host.
OW_DEV float log_f32(float x) {
    if (!(x > 0.0f)) return -3.4028235e38f;  // G6
    if (!(x <= 3.4028235e38f)) return 3.4028235e38f;
    int e = 0;
    if (x < 1.17549435e-38f) {
        x *= 8388608.0f;
        e = -23;
    }
    uint32_t bits;
    __builtin_memcpy(&bits, &x, 4);
    e += (int)(bits >> 23) - 127;
    bits = (bits & 0x007fffffu) | 0x3f800000u;
    float m;
    __builtin_memcpy(&m, &bits, 4);
    if (m > 1.41421354f) {
        m *= 0.5f;
        e += 1;
    }
    const float s = (m - 1.0f) / (m + 1.0f), z = s * s;
    float p = 0.111111111f;
    p = p * z + 0.142857143f;
    p = p * z + 0.2f;
    p = p * z + 0.333333333f;
    p = p * z;                      // s^2/3 + ... + s^8/9
    const float lm = 2.0f * s + (2.0f * s) * p;
    const float fe = (float)e;
    return fe * 0.693145752f + (fe * 1.42860677e-6f + lm);
}

// x^y for x >= 0 and y > 0: 0 at x = 0
OW_DEV float pow_f32(float x, float y) { return x > 0.0f ? exp_f32(y * log_f32(x)) : 0.0f; }

OW_DEV float dot3(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// what the host resolves from ow_render_options: the material, the light and the constants that depend on uniforms alone
struct ShadeParams {
    float water_color[3], foam_color[3];  // linear
    float roughness, normal_strength;     // the uniforms of water.gdshader:14-15
    float fresnel_power;                  // 5 exp(-2.69 roughness), line 92, FP64 on the host and narrowed
    float fresnel_divisor;                // 1 + 22.7 roughness^1.5, line 92, likewise
    float light[3];                       // LIGHT: the unit vector towards the light, world space (normalised in FP64 on the host)
    float light_color[3], ambient_color[3], sky_color[3];
};

// fragment()'s outputs and the varyings light() reads
struct Fragment {
    float dist, wave_height;
    float foam_factor, albedo[3], normal[3], fresnel, roughness;
};

constexpr float kMaskCap = 1e30f;  // stands for GLSL's +Inf in G3 / G4: 1 / (1 + 1e30) is below anything a colour resolves

// water.gdshader:73-93.  `s` is the sample at the solved undisplaced point p (the shader's UV); view_x / view_z are the surface
// position's view-space components along the camera's right and back axes; `view` is the world-space unit vector to the camera.
// This form takes the wave_height varying from the caller (ow_mesh.h: the rasteriser's interpolation of the vertex stage's values).
OW_DEV Fragment shade_fragment(const ShadeParams &sp, const SurfaceSample &s, float wave_height, float view_x, float view_z, const float view[3]) {
    Fragment f;
    f.dist = sqrtf(view_x * view_x + view_z * view_z);                    // :74 length(VERTEX.xz), VERTEX in view space
    f.wave_height = wave_height;                                          // :38 displacement.y, before the distance factor
    float gx = s.gradient_fragment[0], gy = s.gradient_fragment[1];       // :76-84 gradient.xy
    const float gz = s.foam_fragment;                                     //        gradient.z
    const float u = gz * 0.75f, t = u > 0.0f ? (u < 1.0f ? u : 1.0f) : 0.0f;   // :86 smoothstep(0, 1, x): t = clamp(x, 0, 1) ...
    f.foam_factor = (t * t * (3.0f - 2.0f * t)) * exp_f32(-f.dist * 0.0075f);  //     ... t t (3 - 2 t), times exp(-dist 0.0075)
    for (int k = 0; k < 3; ++k) f.albedo[k] = glsl_mix(sp.water_color[k], sp.foam_color[k], f.foam_factor);   // :87
    const float blend = glsl_mix(0.015f, sp.normal_strength, exp_f32(-f.dist * 0.0175f));                     // :89
    gx *= blend;
    gy *= blend;
    const float inv = 1.0f / sqrtf(gx * gx + 1.0f + gy * gy);             // :90 normalize(vec3(-gradient.x, 1, -gradient.y)), world space
    f.normal[0] = -gx * inv;
    f.normal[1] = inv;
    f.normal[2] = -gy * inv;
    float base = 1.0f - dot3(view, f.normal);                             // :92
    base = base > 0.0f ? base : 0.0f;                                     // G1
    f.fresnel = glsl_mix(pow_f32(base, sp.fresnel_power) / sp.fresnel_divisor, 1.0f, 0.02f);   // :92, REFLECTANCE 0.02 (:9)
    f.roughness = (1.0f - f.fresnel) * f.foam_factor + 0.4f;              // :93
    return f;
}
// ... and this one from the sample at the same point: the vertex stage's displacement.y there
OW_DEV Fragment shade_fragment(const ShadeParams &sp, const SurfaceSample &s, float view_x, float view_z, const float view[3]) {
    return shade_fragment(sp, s, s.displacement[1], view_x, view_z, view);
}

// water.gdshader:96-100
OW_DEV float smith_masking_shadowing(float cos_theta, float alpha) {
    const float q = 1.0f - cos_theta * cos_theta;
    const float den = alpha * sqrtf(q > 0.0f ? q : 0.0f);                 // :97, G2
    if (!(den > 0.0f)) return 0.0f;                                       // a = +Inf (or NaN): not below 1.6, :99's else branch
    const float a = cos_theta / den, a_sq = a * a;                        // :97-98
    if (!(a < 1.6f)) return 0.0f;                                         // :99
    const float d = 3.535f * a + 2.181f * a_sq;
    return d > 0.0f ? fminf((1.0f - 1.259f * a + 0.396f * a_sq) / d, kMaskCap) : kMaskCap;   // :99, G3
}

// water.gdshader:103-107
OW_DEV float ggx_distribution(float cos_theta, float alpha) {
    const float a_sq = alpha * alpha;                                     // :104
    const float d = 1.0f + (a_sq - 1.0f) * cos_theta * cos_theta;         // :105
    const float den = 3.14159274f * d * d;                                // :106
    return den > 0.0f ? fminf(a_sq / den, kMaskCap) : (a_sq > 0.0f ? kMaskCap : 0.0f);   // :106, G4
}

struct Lighting {
    float diffuse[3], specular;
};

// water.gdshader:109-127 for one directional light: ATTENUATION = 1 (the material has shadows_disabled, :2)
OW_DEV Lighting shade_light(const ShadeParams &sp, const Fragment &f, const float view[3]) {
    Lighting out;
    float h[3] = {sp.light[0] + view[0], sp.light[1] + view[1], sp.light[2] + view[2]};   // :110
    const float hl = sqrtf(dot3(h, h));
    for (int k = 0; k < 3; ++k) h[k] = hl > 0.0f ? h[k] / hl : 0.0f;      // :110 normalize, G5
    const float dot_nl = fmaxf(dot3(f.normal, sp.light), 2e-5f);          // :111
    const float dot_nv = fmaxf(dot3(f.normal, view), 2e-5f);              // :112
    // the arguments in the order the shader wrote them: (cos_theta, alpha) = (roughness, dot)
    const float light_mask = smith_masking_shadowing(sp.roughness, dot_nv);   // :115
    const float view_mask = smith_masking_shadowing(sp.roughness, dot_nl);    // :116
    const float microfacet = ggx_distribution(dot3(f.normal, h), sp.roughness);   // :117
    const float geometric = 1.0f / (1.0f + light_mask + view_mask);       // :118
    out.specular = f.fresnel * microfacet * geometric / (4.0f * dot_nv + 0.1f);   // :119, no LIGHT_COLOR, as written
    const float sss_modifier[3] = {0.9f, 1.15f, 0.85f};                   // :122
    const float nlv = -dot3(sp.light, view);                              // :123 dot(LIGHT, -VIEW)
    const float c = nlv > 0.0f ? nlv : 0.0f, c2 = c * c;
    const float w = 0.5f - 0.5f * dot3(sp.light, f.normal);
    const float hgt = f.wave_height + 2.5f;
    const float sss_height = (hgt > 0.0f ? hgt : 0.0f) * (c2 * c2) * (w * w * w);   // :123, pow(., 4) and pow(., 3) as products
    const float sss_near = 0.5f * (dot_nv * dot_nv);                      // :124
    const float lambertian = 0.5f * dot_nl;                               // :125
    for (int k = 0; k < 3; ++k) {                                         // :126
        const float lit = (sss_height + sss_near) * sss_modifier[k] / (1.0f + light_mask) + lambertian;
        out.diffuse[k] = glsl_mix(lit, sp.foam_color[k], f.foam_factor) * (1.0f - f.fresnel) * sp.light_color[k];
    }
    return out;
}

}  // namespace ow

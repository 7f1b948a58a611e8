// ow_sky_light.h -- light from the sky over a camera picture (include/ocean_waves.h ow_radiance_*): a roughness-blurred pyramid of the
// panorama, built once from an ow_sky, and a pass over the records that adds the sky's diffuse light and its reflection in the water.
// The counterpart of what the engine does with main.tscn:16-24's PanoramaSkyMaterial: every surface is lit by the sky's irradiance and
// reflects a radiance level chosen by the ROUGHNESS water.gdshader:93 computes.  The frame order becomes
//     water -> solids -> sky light -> ow_environment_apply -> billboards -> ow_present
//
// Compiles as device code (ow_sky_light.hip, built with -ffp-contract=off) and as plain C++ (tests/sky_light/, g++ -ffp-contract=off), like
// ow_environment.h: every FP32 operation is an IEEE-754 add, subtract, multiply, divide or square root, a floor, a conversion or a compare;
// the only transcendentals are exp_f32 (ow_surface.h), atan2_f32 and acos_f32 (ow_environment.h).  Every sine, cosine and sample direction
// is a table the host computes in FP64 and narrows once (radiance_dir_table, radiance_sample_table below: host code, the same in the
// library and in the tests' build).  Both builds therefore produce the same bits for every input.
//
// Everything here is THIS LIBRARY'S CHOICE modelled on Godot's renderer: the engine's source is not part of the reference, so this
// header is the authority for what the calls compute.
//
//   sizes      level 0 starts at the sky's size and is halved while its width exceeds base_width (h halvings); level k is level 0 shifted
//              right by k.  Every halving must be exact (both sides even before it) and every level at least 2 texels wide, else the
//              pyramid is refused (radiance_plan).  A level may be one row high: a 4 x 2 sky has a 2 x 1 level 1.
//   texels     FP32 RGBA, A = 0, rows from the top.
//   P_0        the sky's texels through spray_texel (the sRGB table unless the sky's flag is off), each channel times energy.
//   box        out(i, j) = ((a + b) + (c + d)) 0.25 per channel, a = in(2i, 2j), b = in(2i + 1, 2j), c = in(2i, 2j + 1), d = in(2i + 1, 2j + 1).
//   M_0        box applied h times to P_0 (P_0 itself where h = 0).  M_k = box(M_{k-1}): the unblurred chain.  It runs on past the last
//              level while the width exceeds 64 and both sides are even (the irradiance reads one of its textures).
//   direction  the centre of texel (i, j) of a W x H texture, under ow_environment.h's panorama convention: phi = ((i + 0.5) / W - 0.5) 2 pi,
//              theta = pi (j + 0.5) / H; the column table holds (sin phi, cos phi), the row table (sin theta, cos theta), FP64 narrowed;
//              N = (st sp, ct, -(st cp)) in FP32.
//   samples    for level k >= 1, roughness r = k / (levels - 1), a = r r, and s = 0 .. S - 1 in FP64: xi1 = s / S, xi2 = the radical inverse
//              of s in base 2 (the Hammersley set); ch = sqrt((1 - xi2) / (1 + (a a - 1) xi2)), sh = sqrt(1 - ch ch), the half vector
//              h = (sh cos(2 pi xi1), sh sin(2 pi xi1), ch); with N = V = R = +Z the light vector is l = (2 ch h.x, 2 ch h.y, 2 ch ch - 1)
//              and the weight w = l.z.  The table holds (l.x, l.y, l.z, w) narrowed; a sample whose w is not > 0 is not taken.
//   frame      T = normalise(cross(|N.y| < 0.999 ? +Y : +X, N)), B = cross(N, T): cross products as a b - c d per component, the length
//              as sqrtf((x x + y y) + z z), each component divided by it.
//   tap        tap(M, d) reads a texture along a direction by the sky lookup's own coordinate rule (sky_uv, spray_tap along u: repeat,
//              sky_tap_rows along v: clamp), bilinear on texel centres, the four combined as spray_texture combines them.
//   R_0        = M_0.  R_k(i, j), k >= 1 = (sum_s w_s tap(M_k, d_s)) / sum_s w_s, both sums from 0 in FP32 for s = 0 .. S - 1 in that order
//              on one lane, w_s tap added per channel, d_s = (T l.x + B l.y) + N l.z per component (not renormalised).  If the weights sum
//              to 0, M_k's own texel.
//   E          a 32 x 16 texture.  With M the first texture of the unblurred chain whose width is <= 64 (failing that, the chain's last: the
//              one that could not be halved exactly), n the direction of E's texel and d, st_row those of M's: E = sum w texel / sum w,
//              w = max(dot3(n, d), 0) st_row, over M's texels in row-major order, from 0 in FP32 on one lane; zeros if the weights sum
//              to 0.  A cosine-weighted MEAN: the irradiance over pi, what a diffuse surface of albedo 1 returns.
//
//   the pass   a record WITH kRayHit and WITHOUT kRayEnvironment and kRaySkyLit is processed; every other record is left alone (twice is
//              once; after the fog, nothing).  Only color and status change.  A camera that is not finite (mesh_camera_ok) changes nothing.
//     V        rel = position - camera; len = sqrtf(dot3(rel, rel)); V = -rel / len, or where !(len > 0) the pixel's own ray reversed
//              (env_ray): render_pixel's expressions and fallback.
//     N        the record's normal.  A component that is not finite, or all three 0: no contribution, the bit is still set.
//     ambient  albedo tap(E, N) ambient_energy, per channel ((albedo e) energy).
//     spec     only for water seen from above (neither kRaySolid nor kRayFromBelow), else 0.  nv = dot3(N, V); R = (2 nv) N - V;
//              rc = clamp(roughness, 0, 1) (a NaN: 0); lod = rc (levels - 1); i0 = floorf(lod), frac = lod - i0, i1 = min(i0 + 1, levels - 1);
//              radiance = glsl_mix(tap(R_i0, R), tap(R_i1, R), frac).  The environment BRDF is Karis's analytic fit:
//              r = (rc -1 + 1, rc -0.0275 + 0.0425, rc -0.572 + 1.04, rc 0.022 + -0.04); e = exp_f32((-9.28 max(nv, 0)) ln 2);
//              a004 = min(r.x r.x, e) r.x + r.y; env = (-1.04 a004 + r.z, 1.04 a004 + r.w);
//              spec = (radiance (env.x f0 + env.y f50)) reflection_energy, f0 = (0.16 specular) specular, f50 = clamp(50 f0, 0, 1).
//     color    color + (ambient + spec) per channel; a channel whose result is not finite keeps its old value.
//   The draws' flat ambient_color is still added by the draws: a caller of this pass sets it to 0.
//   out of scope: screen-space reflections, reflection probes, the sky's light on spray (billboards are drawn after the pass).  (The floating
//              bodies' image in the water is ow_mirror.h's pass, which does all of this one and takes its place in the frame order.)
#pragma once

#include <cmath>

#include "ow_environment.h"
#include "ow_solid.h"

namespace ow {

// layout-identical to ow_radiance_options and ow_radiance_light_options in include/ocean_waves.h
struct RadianceOptions {
    int32_t levels, samples, base_width;
    uint32_t reserved[5];
};
struct SkyLightOptions {
    float ambient_energy, reflection_energy, specular;
    uint32_t flags;
    uint32_t reserved[12];
};
static_assert(sizeof(RadianceOptions) == 32 && sizeof(SkyLightOptions) == 64 && offsetof(SkyLightOptions, flags) == 12, "record layout");

constexpr int32_t kRaySkyLit = 64;                    // OW_RAY_SKY_LIT
constexpr int kRadianceMaxLevels = 8;                 // OW_RADIANCE_MAX_LEVELS
constexpr int kRadianceMaxSamples = 256;              // OW_RADIANCE_MAX_SAMPLES
constexpr int kRadianceMinBase = 16, kRadianceMaxBase = 2048;
constexpr int kRadianceDefaultLevels = 6, kRadianceDefaultSamples = 64, kRadianceDefaultBase = 1024;
constexpr int kIrradianceWidth = 32, kIrradianceHeight = 16;
constexpr int kIrradianceSourceWidth = 64;            // the unblurred chain runs on until its width is <= this
constexpr int kRadianceMaxChain = 16;                 // textures of the unblurred chain from M_0 on (a side is at most 8192)
constexpr int kRadianceIrradiance = -1;               // OW_RADIANCE_IRRADIANCE: ow_radiance_level's name for E
constexpr float kSkyLightEnergyMax = 1.0e12f;         // the largest ambient_energy and reflection_energy

// ---- sizes -------------------------------------------------------------------------------------------------------------------------------

// where everything of a pyramid is, in texels
struct RadiancePlan {
    int levels, samples;
    int pre;                                         // halvings from the sky's size to level 0's
    int chain;                                       // textures of the unblurred chain M_0 .. M_{chain-1}; chain >= levels
    int source;                                      // the M_k the irradiance reads
    int width[kRadianceMaxChain], height[kRadianceMaxChain];  // of M_k (and of R_k for k < levels)
};
// false: a halving would have to round, or a level is narrower than 2 texels
inline bool radiance_plan(int sky_width, int sky_height, int levels, int base_width, RadiancePlan *p) {
    int w = sky_width, h = sky_height;
    p->levels = levels;
    p->pre = 0;
    while (w > base_width) {
        if ((w & 1) || (h & 1)) return false;
        w >>= 1;
        h >>= 1;
        ++p->pre;
    }
    p->chain = 0;
    for (;;) {
        if (w < 2 || h < 1) return false;
        p->width[p->chain] = w;
        p->height[p->chain] = h;
        ++p->chain;
        const bool even = !(w & 1) && !(h & 1);
        if (p->chain < levels) {
            if (!even) return false;
        } else if (w <= kIrradianceSourceWidth || !even || w < 4 || p->chain == kRadianceMaxChain) {
            break;
        }
        w >>= 1;
        h >>= 1;
    }
    p->source = p->chain - 1;
    for (int k = p->chain - 1; k >= 0; --k)
        if (p->width[k] <= kIrradianceSourceWidth) p->source = k;
    return true;
}

// ---- the host's tables (FP64, narrowed once) ---------------------------------------------------------------------------------------------

// (sin, cos) pairs: n column entries, phi = ((i + 0.5) / n - 0.5) 2 pi, or n row entries, theta = pi (j + 0.5) / n
inline void radiance_dir_table(int n, bool rows, float *out) {
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < n; ++i) {
        const double a = rows ? pi * (((double)i + 0.5) / (double)n) : (((double)i + 0.5) / (double)n - 0.5) * (2.0 * pi);
        out[2 * i] = (float)std::sin(a);
        out[2 * i + 1] = (float)std::cos(a);
    }
}
// (l.x, l.y, l.z, w) of the S GGX importance samples at roughness r
inline void radiance_sample_table(double r, int S, float *out) {
    const double pi = 3.14159265358979323846;
    const double a = r * r;
    for (int s = 0; s < S; ++s) {
        double xi2 = 0.0, f = 0.5;
        for (unsigned b = (unsigned)s; b; b >>= 1, f *= 0.5)
            if (b & 1u) xi2 += f;
        const double xi1 = (double)s / (double)S;
        const double ch = std::sqrt((1.0 - xi2) / (1.0 + (a * a - 1.0) * xi2));
        const double sh = std::sqrt(1.0 - ch * ch > 0.0 ? 1.0 - ch * ch : 0.0);
        const double phi = 2.0 * pi * xi1;
        const double hx = sh * std::cos(phi), hy = sh * std::sin(phi);
        const double lz = 2.0 * ch * ch - 1.0;
        out[4 * s] = (float)(2.0 * ch * hx);
        out[4 * s + 1] = (float)(2.0 * ch * hy);
        out[4 * s + 2] = (float)lz;
        out[4 * s + 3] = (float)lz;
    }
}

// ---- lane code ---------------------------------------------------------------------------------------------------------------------------

// an FP32 RGBA texture, rows from the top
struct RadianceLevel {
    const float *texels;  // [height][width][4]
    int width, height;
};

OW_DEV void radiance_cross(const float a[3], const float b[3], float out[3]) {
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}
// the direction of a texel centre from its column and row entries
OW_DEV void radiance_texel_dir(const float *col, const float *row, int i, int j, float n[3]) {
    const float sp = col[2 * i], cp = col[2 * i + 1], st = row[2 * j], ct = row[2 * j + 1];
    n[0] = st * sp;
    n[1] = ct;
    n[2] = -(st * cp);
}
OW_DEV void radiance_frame(const float n[3], float t[3], float b[3]) {
    const float y[3] = {0.0f, 1.0f, 0.0f}, x[3] = {1.0f, 0.0f, 0.0f};
    float c[3];
    radiance_cross(fabsf(n[1]) < 0.999f ? y : x, n, c);
    const float len = sqrtf((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    for (int k = 0; k < 3; ++k) t[k] = c[k] / len;
    radiance_cross(n, t, b);
}
// a texture along a direction: the sky lookup's coordinates and weights (ow_environment.h sky_texture) over FP32 texels
OW_DEV void radiance_tap(const RadianceLevel &t, const float d[3], float out[3]) {
    float u, v;
    sky_uv(d, u, v);
    int x0, x1, y0, y1;
    float wx, wy;
    spray_tap(u, t.width, x0, x1, wx);
    sky_tap_rows(v, t.height, y0, y1, wy);
    const float *a = t.texels + 4 * ((size_t)y0 * t.width + x0), *b = t.texels + 4 * ((size_t)y0 * t.width + x1);
    const float *c = t.texels + 4 * ((size_t)y1 * t.width + x0), *e = t.texels + 4 * ((size_t)y1 * t.width + x1);
    const float ux = 1.0f - wx, uy = 1.0f - wy;
    for (int k = 0; k < 3; ++k) out[k] = (a[k] * ux + b[k] * wx) * uy + (c[k] * ux + e[k] * wx) * wy;
}

// P_0: texel (i, j) of the sky, decoded, times the energy
OW_DEV void radiance_decode_texel(const SprayTexture &sky, const float *srgb, float energy, int i, int j, float out[4]) {
    float t[4];
    spray_texel(sky, srgb, i, j, t);
    for (int k = 0; k < 3; ++k) out[k] = t[k] * energy;
    out[3] = 0.0f;
}
// the 2 x 2 box: texel (i, j) of the half-size texture from `in` (in_width texels a row)
OW_DEV void radiance_box_texel(const float *in, int in_width, int i, int j, float out[4]) {
    const float *a = in + 4 * ((size_t)(2 * j) * in_width + 2 * i), *c = a + 4 * (size_t)in_width;
    for (int k = 0; k < 3; ++k) out[k] = ((a[k] + a[4 + k]) + (c[k] + c[4 + k])) * 0.25f;
    out[3] = 0.0f;
}
// R_k(i, j) from M_k (m), its column and row tables and the level's S samples
OW_DEV void radiance_prefilter_texel(const RadianceLevel &m, const float *col, const float *row, const float *samples, int S, int i, int j, float out[4]) {
    float n[3], t[3], b[3];
    radiance_texel_dir(col, row, i, j, n);
    radiance_frame(n, t, b);
    float sum[3] = {0.0f, 0.0f, 0.0f}, wsum = 0.0f;
    for (int s = 0; s < S; ++s) {
        const float *l = samples + 4 * s;
        const float w = l[3];
        if (!(w > 0.0f)) continue;
        float d[3], c[3];
        for (int k = 0; k < 3; ++k) d[k] = (t[k] * l[0] + b[k] * l[1]) + n[k] * l[2];
        radiance_tap(m, d, c);
        for (int k = 0; k < 3; ++k) sum[k] += w * c[k];
        wsum += w;
    }
    const float *own = m.texels + 4 * ((size_t)j * m.width + i);
    for (int k = 0; k < 3; ++k) out[k] = wsum > 0.0f ? sum[k] / wsum : own[k];
    out[3] = 0.0f;
}
// E(i, j) from its source in the unblurred chain (m) and that texture's tables; ecol, erow: E's own
OW_DEV void radiance_irradiance_texel(const RadianceLevel &m, const float *col, const float *row, const float *ecol, const float *erow, int i, int j,
                                      float out[4]) {
    float n[3];
    radiance_texel_dir(ecol, erow, i, j, n);
    float sum[3] = {0.0f, 0.0f, 0.0f}, wsum = 0.0f;
    for (int y = 0; y < m.height; ++y)
        for (int x = 0; x < m.width; ++x) {
            float d[3];
            radiance_texel_dir(col, row, x, y, d);
            const float c = dot3(n, d);
            const float w = (c > 0.0f ? c : 0.0f) * row[2 * y];
            const float *t = m.texels + 4 * ((size_t)y * m.width + x);
            for (int k = 0; k < 3; ++k) sum[k] += w * t[k];
            wsum += w;
        }
    for (int k = 0; k < 3; ++k) out[k] = wsum > 0.0f ? sum[k] / wsum : 0.0f;
    out[3] = 0.0f;
}

// what a build works on: the sky (borrowed until the build has run), the plan and where each texture and table lies on the device
struct RadianceBuild {
    SprayTexture sky;
    const float *srgb;                    // [256] spray_srgb_table
    float energy;
    RadiancePlan plan;
    float *pre[16];                       // P_0 .. P_{pre-1}: the sizes above level 0's (scratch)
    float *M[kRadianceMaxChain];          // the unblurred chain; M[0] is R[0]
    float *R[kRadianceMaxLevels];
    const float *col[kRadianceMaxChain], *row[kRadianceMaxChain];  // the direction tables of M_k's size
    const float *samples[kRadianceMaxLevels];                      // [S][4] per level from 1 on
    float *E;
    const float *ecol, *erow;             // E's own direction tables
};

// ---- the pass ----------------------------------------------------------------------------------------------------------------------------

// a pass's constants, resolved once from the options and the pyramid
struct SkyLightParams {
    int camera_ok;  // 0: the camera is not finite -- nothing changes
    int levels;
    float ambient_energy, reflection_energy;
    float f0, f50;  // (0.16 specular) specular and clamp(50 f0, 0, 1), FP32
    RadianceLevel R[kRadianceMaxLevels];
    RadianceLevel E;
};
inline void sky_light_fresnel(float specular, float &f0, float &f50) {  // host code
    f0 = (0.16f * specular) * specular;
    const float v = 50.0f * f0;
    f50 = v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f;
}

// what the pass makes of one record, with the intermediates the tests read (zeros where a stage was not reached)
struct SkyLightPixel {
    bool changed;       // color and status are to be written
    int32_t status;
    float color[3];
    float view[3], reflect[3];
    float lod;
    float radiance[3];
    float env[2];
    float irradiance[3], ambient[3], spec[3];
};
// The pass's work on one record, in two parts so that ow_mirror.h's pass can put a body's image into px.radiance between them; sky_light_pixel
// below is the two in a row.  sky_light_begin runs up to radiance and env and says how far the record goes:
enum : int {
    kSkyLightLeft = 0,     // not processed: nothing is written
    kSkyLightMarked = 1,   // processed, no contribution (the normal is zero or not finite)
    kSkyLightAmbient = 2,  // ambient only (a solid, or water seen from below)
    kSkyLightWater = 3     // water seen from above: reflect, lod, radiance and env are set, spec is sky_light_finish's
};
OW_DEV int sky_light_begin(const SkyLightParams &lp, const CameraParams &cam, int i, int j, int32_t status, const float position[3], const float albedo[3],
                           const float normal[3], float roughness, const float color[3], SkyLightPixel &px) {
    px.changed = false;
    px.status = status;
    px.lod = 0.0f;
    px.env[0] = px.env[1] = 0.0f;
    for (int k = 0; k < 3; ++k) {
        px.color[k] = color[k];
        px.view[k] = px.reflect[k] = px.radiance[k] = px.irradiance[k] = px.ambient[k] = px.spec[k] = 0.0f;
    }
    if (!lp.camera_ok || !(status & kRayHit) || (status & (kRayEnvironment | kRaySkyLit))) return kSkyLightLeft;
    px.changed = true;
    px.status = status | kRaySkyLit;
    bool ok = true, zero = true;
    for (int k = 0; k < 3; ++k) {
        ok = ok && mesh_finite(normal[k]);
        zero = zero && normal[k] == 0.0f;
    }
    if (!ok || zero) return kSkyLightMarked;
    float rel[3];
    for (int k = 0; k < 3; ++k) rel[k] = position[k] - cam.o[k];
    const float len = sqrtf(dot3(rel, rel));
    if (len > 0.0f) {
        for (int k = 0; k < 3; ++k) px.view[k] = -rel[k] / len;
    } else {
        float d[3];
        env_ray(cam, i, j, d);
        for (int k = 0; k < 3; ++k) px.view[k] = -d[k];
    }
    radiance_tap(lp.E, normal, px.irradiance);
    for (int k = 0; k < 3; ++k) px.ambient[k] = (albedo[k] * px.irradiance[k]) * lp.ambient_energy;
    if (status & (kRaySolid | kRayFromBelow)) return kSkyLightAmbient;
    const float nv = dot3(normal, px.view);
    for (int k = 0; k < 3; ++k) px.reflect[k] = (2.0f * nv) * normal[k] - px.view[k];
    const float rc = env_clamp01(roughness);
    px.lod = rc * (float)(lp.levels - 1);
    const float l0 = floorf(px.lod), frac = px.lod - l0;
    const int i0 = (int)l0, i1 = i0 + 1 > lp.levels - 1 ? lp.levels - 1 : i0 + 1;
    float r0[3], r1[3];
    radiance_tap(lp.R[i0], px.reflect, r0);
    radiance_tap(lp.R[i1], px.reflect, r1);
    for (int k = 0; k < 3; ++k) px.radiance[k] = glsl_mix(r0[k], r1[k], frac);
    const float rx = rc * -1.0f + 1.0f, ry = rc * -0.0275f + 0.0425f, rz = rc * -0.572f + 1.04f, rw = rc * 0.022f + -0.04f;
    const float e = exp_f32((-9.28f * (nv > 0.0f ? nv : 0.0f)) * 0.693147182f);
    const float rx2 = rx * rx;
    const float a004 = (rx2 < e ? rx2 : e) * rx + ry;
    px.env[0] = -1.04f * a004 + rz;
    px.env[1] = 1.04f * a004 + rw;
    return kSkyLightWater;
}
// from `scale` on: spec from px.radiance and px.env (kSkyLightWater), then color
OW_DEV void sky_light_finish(const SkyLightParams &lp, const float color[3], int stage, SkyLightPixel &px) {
    if (stage < kSkyLightAmbient) return;
    if (stage == kSkyLightWater) {
        const float scale = px.env[0] * lp.f0 + px.env[1] * lp.f50;
        for (int k = 0; k < 3; ++k) px.spec[k] = (px.radiance[k] * scale) * lp.reflection_energy;
    }
    for (int k = 0; k < 3; ++k) {
        const float v = color[k] + (px.ambient[k] + px.spec[k]);
        px.color[k] = mesh_finite(v) ? v : color[k];
    }
}
OW_DEV SkyLightPixel sky_light_pixel(const SkyLightParams &lp, const CameraParams &cam, int i, int j, int32_t status, const float position[3],
                                     const float albedo[3], const float normal[3], float roughness, const float color[3]) {
    SkyLightPixel px;
    const int stage = sky_light_begin(lp, cam, i, j, status, position, albedo, normal, roughness, color, px);
    sky_light_finish(lp, color, stage, px);
    return px;
}

}  // namespace ow

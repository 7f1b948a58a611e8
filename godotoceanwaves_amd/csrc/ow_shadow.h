// ow_shadow.h -- the floating bodies' sun shadows (include/ocean_waves.h ow_shadow_*): a depth map of the casters as the light sees them, and
// a pass over the records of a picture that darkens the sun's share of each by it.
//
// Compiles as device code (ow_shadow.hip, built with -ffp-contract=off) and as plain C++ (tests/shadow/, g++ -ffp-contract=off), like
// ow_solid.h: every operation is an IEEE-754 add, subtract, multiply, divide, min / max or compare, in FP32 or (where stated) FP64, so both
// builds produce the same bits.  This header is the authority wherever the text in include/ocean_waves.h leaves an order of operations open.
//
// All of this is THIS LIBRARY'S CHOICE, modelled on the engine's directional shadow (an orthographic depth map from the light, a normal
// bias that grows with the slope, a filtered depth comparison); the engine's source is not part of the reference.  The scene's settings
// (main.tscn:114-117) are taken where they have a meaning here: shadow_bias, shadow_normal_bias and shadow_opacity.  shadow_blur 5 has no
// unit to carry over -- the engine scales it by its own soft-shadow kernel and the cascade's texel size -- so the filter's width is an
// option of its own (filter_taps).
//
//   frame     the host normalises light_direction in FP64 (as ow_shading.h's light is) and builds the basis there: z = l^,
//             x = normalize((0,1,0) x z) (x = (1,0,0) where z.x^2 + z.z^2 < 1e-6), y = z x x, each narrowed once.  For a world point w:
//             r_k = w_k - center_k; u = dot3(x, r); v = dot3(y, r); d = depth_range - dot3(z, r) (metres from the frame's near plane, growing
//             away from the light); s = u k + half, t = v k + half with k = size / (2 half_extent) narrowed once and half = size / 2.
//             Texel (i, j) has its centre at (i + 0.5, j + 0.5).
//   vertex    world position: ow_solid.h's solid_world, the function the draw's solid_vertex calls; the skip rule is solid_instance_ok's.
//             A vertex whose world position or (s, t, d) is not finite is flagged; its triangles are culled.
//   facing    A = (s1 - s0)(t2 - t0) - (s2 - s0)(t1 - t0): the differences in FP32, the products and their difference in FP64.  A > 0 is a
//             triangle whose outward side is turned towards the light.  Only A < 0 is cast unless both sides are asked for: the faces
//             of a closed body that the light reaches never enter the map, so a body cannot shadow its own lit faces whatever the bias.
//             That is why the scene's shadow_bias 0 is safe here.  A = 0 is never cast.
//   box       the texels whose centres may be covered: i from max(floorf(min s - 0.5), 0) to min(ceilf(max s - 0.5), size - 1), j likewise.
//             An empty box (outside the footprint) is culled, and so is a triangle whose three depths all exceed 2 depth_range.  Every
//             other triangle counts as drawn (a box of at most lane_box texels a side: the lane class, otherwise the wave class).
//   coverage  at the centre p: e0 = (s2 - s1)(p.y - t1) - (t2 - t1)(p.x - s1), e1 = (s0 - s2)(p.y - t2) - (t0 - t2)(p.x - s2),
//             e2 = (s1 - s0)(p.y - t0) - (t1 - t0)(p.x - s0): FP32 differences, FP64 products and difference.  Covered when all three have
//             A's sign or are 0 (inclusive on both sides of every edge) and E = (e0 + e1) + e2 is not 0.
//   depth     ((e0 / E) d0 + (e1 / E) d1) + (e2 / E) d2 in FP64, narrowed once, then fmaxf(., 0).  Written when finite and <= 2 depth_range:
//             the smaller of it and the word that is there (the FP32 bits of positive floats order as unsigned integers).
//   receiver  a record with kRayHit and with neither kRayShadowed nor kRayEnvironment; kRaySolid records always, water records only when
//             the options say so.  ndl = fmaxf(dot3(normal, l^), 0); o = ((1 - ndl) normal_bias) w, w = 2 half_extent / size (FP64 on the
//             host, narrowed once); P'_k = position_k + normal_k o; (s, t, d) of P'; d_r = d - bias w.
//   filter    r = (taps - 1) / 2.  sx = s - 0.5, i0 = floorf(sx), fx = sx - i0 (t likewise).  Taps i0 - r .. i0 + r + 1 on each axis with the
//             weights 1 - fx, 1 .. 1, fx.  lit = d_r <= D_tap; a tap outside the map is lit.  acc = sum over rows, then along each row, of
//             (w_x w_y) where lit, in FP32.  V = 1 when no tap of non-zero weight is unlit, 0 when none is lit, else
//             fminf(acc / (2r + 1)^2, 1).  A receiver whose s, t or d_r is not finite, or that lies more than the filter's reach outside the
//             map, has V = 1.
//   record    a = opacity (1 - V); per channel color' = color - a (albedo diffuse + specular), diffuse' = diffuse (1 - a),
//             specular' = specular (1 - a); a value that would not be finite keeps what it had.  status gets kRayShadowed.
#pragma once

#include <cmath>

#include "ow_render.h"
#include "ow_solid.h"

namespace ow {

// layout-identical to ow_shadow_frame in include/ocean_waves.h
struct ShadowFrame {
    float light_direction[3];
    float half_extent;
    float center[3];
    float depth_range;
    uint32_t flags;
    int32_t lane_box;
    uint32_t reserved[6];
};
// layout-identical to ow_shadow_options in include/ocean_waves.h
struct ShadowOptions {
    float bias, normal_bias, opacity;
    int32_t filter_taps;
    uint32_t flags;
    uint32_t reserved[11];
};
static_assert(sizeof(ShadowFrame) == 64 && offsetof(ShadowFrame, center) == 16 && offsetof(ShadowFrame, flags) == 32 && sizeof(ShadowOptions) == 64 &&
                  offsetof(ShadowOptions, flags) == 16,
              "record layout");

constexpr int32_t kRayShadowed = 128;           // OW_RAY_SHADOWED
constexpr int32_t kRayEnvironmentDone = 32;     // OW_RAY_ENVIRONMENT (ow_environment.h's flag, restated: this header does not need the pass)
constexpr uint32_t kShadowCastBothSides = 1u;   // OW_SHADOW_CAST_BOTH_SIDES
constexpr uint32_t kShadowReceiveWater = 1u;    // OW_SHADOW_RECEIVE_WATER
constexpr int kShadowMinSize = 8, kShadowMaxSize = 8192;
constexpr uint32_t kShadowEmpty = 0x7f7fffffu;  // FLT_MAX's bits
constexpr uint32_t kShadowVertexNotFinite = 1u, kShadowVertexSkipped = 2u;
constexpr float kShadowRangeMax = 1.0e6f;       // half_extent, depth_range and the biases

// what the four counters of a map hold since its last begin: skipped instances, then every triangle of the other instances as one of three
enum : int { kShadowSkippedInstances = kSolidSkippedInstances, kShadowCulled = kSolidCulled, kShadowLane = kSolidLane, kShadowWave = kSolidWave };
enum : int { kShadowTriNone = -1, kShadowTriSkipped = 0, kShadowTriCulled = 1, kShadowTriLane = 2, kShadowTriWave = 3 };

// a frame as the host resolves it for a map of side `size`
struct ShadowParams {
    float x[3], y[3], z[3];  // the basis; z is the unit vector towards the light
    float center[3];
    float depth_range, max_depth;  // max_depth = 2 depth_range
    float k, half, w;        // texels per metre, size / 2, metres per texel
    int size;
    int both_sides, lane_box;
    int ok;                  // 0: no frame, or one that is not finite -- nothing is cast and nothing is shadowed
};

// the pass's constants, resolved from the options
struct ShadowApply {
    float bias, normal_bias, opacity;
    int r;                   // the filter's radius: taps = 2 r + 1
    int receive_water;
    int camera_ok;
};

// Host code (FP64, square roots): the frame's constants for a map of side `size`.  ok = 0 for a frame that is not finite, out of its
// ranges or without a direction; the entry points refuse those with a message before they get here.
inline ShadowParams shadow_params(const ShadowFrame &f, int size) {
    ShadowParams P;
    __builtin_memset(&P, 0, sizeof(P));
    P.size = size;
    bool ok = f.half_extent > 0.0f && f.half_extent <= kShadowRangeMax && f.depth_range > 0.0f && f.depth_range <= kShadowRangeMax;
    for (int k = 0; k < 3; ++k) ok = ok && mesh_finite(f.light_direction[k]) && mesh_finite(f.center[k]);
    const double lx = f.light_direction[0], ly = f.light_direction[1], lz = f.light_direction[2];
    const double len = sqrt(lx * lx + ly * ly + lz * lz);
    if (!ok || !(len > 0.0)) return P;
    const double z[3] = {lx / len, ly / len, lz / len};
    double x[3] = {1.0, 0.0, 0.0};
    const double h2 = z[0] * z[0] + z[2] * z[2];
    if (!(h2 < 1e-6)) {  // (0,1,0) x z = (z.z, 0, -z.x)
        const double h = sqrt(h2);
        x[0] = z[2] / h;
        x[2] = -z[0] / h;
    }
    const double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
    for (int k = 0; k < 3; ++k) {
        P.x[k] = (float)x[k];
        P.y[k] = (float)y[k];
        P.z[k] = (float)z[k];
        P.center[k] = f.center[k];
    }
    P.depth_range = f.depth_range;
    P.max_depth = 2.0f * f.depth_range;
    P.k = (float)((double)size / (2.0 * (double)f.half_extent));
    P.half = (float)((double)size / 2.0);
    P.w = (float)(2.0 * (double)f.half_extent / (double)size);
    P.both_sides = (f.flags & kShadowCastBothSides) ? 1 : 0;
    P.lane_box = mesh_lane_box(f.lane_box);
    P.ok = 1;
    return P;
}
// ... and the pass's, from options the entry points have checked (filter_taps 0 selects 5)
inline ShadowApply shadow_apply_params(const ShadowOptions &o, bool camera_ok) {
    ShadowApply ap;
    ap.bias = o.bias;
    ap.normal_bias = o.normal_bias;
    ap.opacity = o.opacity;
    ap.r = ((o.filter_taps == 0 ? 5 : o.filter_taps) - 1) / 2;
    ap.receive_water = (o.flags & kShadowReceiveWater) ? 1 : 0;
    ap.camera_ok = camera_ok ? 1 : 0;
    return ap;
}

// one (instance, vertex) in the light's frame: 16 bytes
struct ShadowVertex {
    float s, t, d;
    uint32_t flags;
};
static_assert(sizeof(ShadowVertex) == 16, "one 16-byte store");

OW_DEV void shadow_project(const ShadowParams &P, const float w[3], float &s, float &t, float &d) {
    float r[3];
    for (int k = 0; k < 3; ++k) r[k] = w[k] - P.center[k];
    const float u = dot3(P.x, r), v = dot3(P.y, r);
    d = P.depth_range - dot3(P.z, r);
    s = u * P.k + P.half;
    t = v * P.k + P.half;
}

OW_DEV ShadowVertex shadow_vertex(const float *t, bool instance_ok, const float l[3], const ShadowParams &P) {
    ShadowVertex out;
    out.s = out.t = out.d = 0.0f;
    if (!instance_ok) {
        out.flags = kShadowVertexNotFinite | kShadowVertexSkipped;
        return out;
    }
    float w[3];
    bool ok = solid_world(t, l, w);
    float s, tt, d;
    shadow_project(P, w, s, tt, d);
    ok = ok && mesh_finite(s) && mesh_finite(tt) && mesh_finite(d);
    out.flags = ok ? 0u : kShadowVertexNotFinite;
    if (ok) {
        out.s = s;
        out.t = tt;
        out.d = d;
    }
    return out;
}

// a triangle ready for the walk: nine floats and four integers, all a lane read can carry
struct ShadowSetup {
    float s[3], t[3], d[3];
    int x0, x1, y0, y1;
    int kind;  // kShadowTri*
};

OW_DEV double shadow_area(const float s[3], const float t[3]) {
    return (double)(s[1] - s[0]) * (double)(t[2] - t[0]) - (double)(s[2] - s[0]) * (double)(t[1] - t[0]);
}

OW_DEV ShadowSetup shadow_setup(const ShadowVertex &a, const ShadowVertex &b, const ShadowVertex &c, const ShadowParams &P) {
    ShadowSetup S;
    S.s[0] = a.s, S.s[1] = b.s, S.s[2] = c.s;
    S.t[0] = a.t, S.t[1] = b.t, S.t[2] = c.t;
    S.d[0] = a.d, S.d[1] = b.d, S.d[2] = c.d;
    S.x0 = S.y0 = 0;
    S.x1 = S.y1 = -1;
    const uint32_t f = a.flags | b.flags | c.flags;
    if (f & kShadowVertexSkipped) {
        S.kind = kShadowTriSkipped;
        return S;
    }
    S.kind = kShadowTriCulled;
    if (f) return S;
    const double A = shadow_area(S.s, S.t);
    if (!(P.both_sides ? A != 0.0 : A < 0.0)) return S;
    if (fminf(fminf(S.d[0], S.d[1]), S.d[2]) > P.max_depth) return S;
    const float top = (float)(P.size - 1);
    const float lo_x = fmaxf(floorf(fminf(fminf(S.s[0], S.s[1]), S.s[2]) - 0.5f), 0.0f), hi_x = fminf(ceilf(fmaxf(fmaxf(S.s[0], S.s[1]), S.s[2]) - 0.5f), top);
    const float lo_y = fmaxf(floorf(fminf(fminf(S.t[0], S.t[1]), S.t[2]) - 0.5f), 0.0f), hi_y = fminf(ceilf(fmaxf(fmaxf(S.t[0], S.t[1]), S.t[2]) - 0.5f), top);
    if (!(lo_x <= hi_x && lo_y <= hi_y)) return S;
    S.x0 = (int)lo_x, S.x1 = (int)hi_x, S.y0 = (int)lo_y, S.y1 = (int)hi_y;
    S.kind = (S.x1 - S.x0 < P.lane_box && S.y1 - S.y0 < P.lane_box) ? kShadowTriLane : kShadowTriWave;
    return S;
}

// the texel centre (i + 0.5, j + 0.5) against one triangle: covered, and the depth's bits
struct ShadowCover {
    bool hit;
    uint32_t bits;
};
OW_DEV ShadowCover shadow_cover(const float s[3], const float t[3], const float d[3], float max_depth, int i, int j) {
    ShadowCover c;
    c.hit = false;
    c.bits = kShadowEmpty;
    const float px = (float)i + 0.5f, py = (float)j + 0.5f;
    const double A = shadow_area(s, t);
    const double e0 = (double)(s[2] - s[1]) * (double)(py - t[1]) - (double)(t[2] - t[1]) * (double)(px - s[1]);
    const double e1 = (double)(s[0] - s[2]) * (double)(py - t[2]) - (double)(t[0] - t[2]) * (double)(px - s[2]);
    const double e2 = (double)(s[1] - s[0]) * (double)(py - t[0]) - (double)(t[1] - t[0]) * (double)(px - s[0]);
    const bool in = A > 0.0 ? (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) : (A < 0.0 && e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0);
    if (!in) return c;
    const double E = (e0 + e1) + e2;
    if (E == 0.0) return c;
    const float depth = fmaxf((float)(((e0 / E) * (double)d[0] + (e1 / E) * (double)d[1]) + (e2 / E) * (double)d[2]), 0.0f);
    if (!(depth <= max_depth)) return c;  // false for a NaN; max_depth is finite
    c.hit = true;
    c.bits = __builtin_bit_cast(uint32_t, depth);
    return c;
}

// the light's visibility of a receiver: d_r against the map's words under the filter
OW_DEV float shadow_visibility(const ShadowParams &P, int r, const uint32_t *map, float s, float t, float d_r) {
    if (!(mesh_finite(s) && mesh_finite(t) && mesh_finite(d_r))) return 1.0f;
    const float sx = s - 0.5f, sy = t - 0.5f;
    const float reach = (float)(r + 2), far = (float)P.size + reach;
    if (!(sx >= -reach && sx <= far && sy >= -reach && sy <= far)) return 1.0f;
    const float fi = floorf(sx), fj = floorf(sy);
    const float fx = sx - fi, fy = sy - fj;
    const int i0 = (int)fi, j0 = (int)fj;
    float acc = 0.0f;
    bool any_lit = false, any_unlit = false;
    for (int b = -r; b <= r + 1; ++b) {
        const float wy = b == -r ? 1.0f - fy : (b == r + 1 ? fy : 1.0f);
        const int j = j0 + b;
        for (int a = -r; a <= r + 1; ++a) {
            const float wx = a == -r ? 1.0f - fx : (a == r + 1 ? fx : 1.0f);
            const int i = i0 + a;
            bool lit = true;
            if (i >= 0 && i < P.size && j >= 0 && j < P.size) lit = d_r <= __builtin_bit_cast(float, map[(size_t)j * P.size + i]);
            const float w = wx * wy;
            if (lit) acc = acc + w;
            if (w > 0.0f) {
                any_lit = any_lit || lit;
                any_unlit = any_unlit || !lit;
            }
        }
    }
    if (!any_unlit) return 1.0f;
    if (!any_lit) return 0.0f;
    const float n = (float)((2 * r + 1) * (2 * r + 1));
    return fminf(acc / n, 1.0f);
}

OW_DEV bool shadow_receives(const ShadowApply &ap, int32_t status) {
    if (!(status & kRayHit) || (status & (kRayShadowed | kRayEnvironmentDone))) return false;
    return (status & kRaySolid) || ap.receive_water;
}

// One record.  Reads status, position, albedo, normal, diffuse, specular and color; rewrites status, diffuse, specular and color of a
// receiver (true) and nothing of any other record (false).  V: the receiver's visibility.
OW_DEV bool shadow_record(const ShadowParams &P, const ShadowApply &ap, const uint32_t *map, RenderPixel &px, float &V) {
    V = 1.0f;
    if (!P.ok || !ap.camera_ok || !shadow_receives(ap, px.status)) return false;
    const float ndl = fmaxf(dot3(px.normal, P.z), 0.0f);
    const float o = ((1.0f - ndl) * ap.normal_bias) * P.w;
    float w[3];
    for (int k = 0; k < 3; ++k) w[k] = px.position[k] + px.normal[k] * o;
    float s, t, d;
    shadow_project(P, w, s, t, d);
    const float d_r = d - ap.bias * P.w;
    V = shadow_visibility(P, ap.r, map, s, t, d_r);
    const float a = ap.opacity * (1.0f - V), keep = 1.0f - a;
    for (int k = 0; k < 3; ++k) {
        const float c = px.color[k] - a * (px.albedo[k] * px.diffuse[k] + px.specular);
        const float df = px.diffuse[k] * keep;
        if (mesh_finite(c)) px.color[k] = c;
        if (mesh_finite(df)) px.diffuse[k] = df;
    }
    const float sp = px.specular * keep;
    if (mesh_finite(sp)) px.specular = sp;
    px.status |= kRayShadowed;
    return true;
}

}  // namespace ow

// ow_mist.h -- height mist with sun shafts over a camera picture (include/ocean_waves.h ow_mist_*): the sea mist of the reference scene's
// volumetric fog (main.tscn:35-37) and its world-sized FogVolume (:100-104, :142-144), whose FogMaterial's density falls off with height
// (height_falloff = 0.176), lit by the low Sun (:113) and cut by the crates' shadows out of the resident depth map (ow_shadow.h).
//
// Compiles as device code (ow_mist.hip, built with -ffp-contract=off) and as plain C++ (tests/mist/, g++ -ffp-contract=off), like
// ow_shadow.h: every FP32 operation is an IEEE-754 add, subtract, multiply, divide or square root, a conversion or a compare; exp is
// exp_f32 (ow_surface.h).  There is no library transcendental, so both builds produce the same bits for every input.
//
// All of this is THIS LIBRARY'S CHOICE, modelled on the engine's volumetric fog (froxels along the view ray spread towards the eye, a
// Henyey-Greenstein phase function, one shadow-map compare per froxel); the engine's source is not part of the reference, so this header
// is the authority for what the calls compute.
//
//   medium     for a camera ray from o along the unit direction d: h(t) = (o.y - base_height) + t d.y; the weight is w(h) = 1 for h <= 0
//              and exp(-k h) above, k = height_falloff ln 2 (FP64 on the host, narrowed once): FogMaterial's
//              clamp(exp2(-height_falloff (y - y_object)), 0, 1).  I(t) = integral of w(h(s)) over [0, t], T(t) = exp_f32(-(extinction I(t))).
//   integral   per segment as LENGTH x MEAN WEIGHT, never as a difference of antiderivatives (which cancels for near-horizontal rays):
//              a segment wholly at or below the base has mean 1; one wholly above it, between the heights lo <= hi, has mean
//              exp_f32(-(k lo)) phi(k (hi - lo)), phi(x) = (1 - exp_f32(-x)) / x, for x < 0.5 its series through x^8 / 9! (Horner); one that
//              crosses the base is split at t_c = -h(0) / d.y, clamped to [0, t]: I = below + above phi(k hi), hi the height of the end above.
//   ray        ow_environment.h's env_ray.  t_end = min(record.t, length) for a record with kRayHit (a t that is not > 0 counts as 0),
//              length otherwise.  N = slices (0 selects 64).  Boundaries t_i = t_end (f f) with f = (float)i / (float)N (the engine's detail
//              spread of 2 puts the slices near the eye); midpoints m_i = 0.5 (t_i + t_{i+1}).
//   shafts     V_i: ONE depth compare of the world point o + m_i d (per component o_k + m_i d_k) in the shadow map: ow_shadow.h's
//              shadow_project as it is, the texel containing (s, t), lit when d - shadow_bias w <= D.  A point outside the footprint,
//              beyond 2 depth_range, not finite, with a NULL map, or with a map that has had no ow_shadow_map_begin is lit.
//   pixel      A = 1 - T(t_end), clamped to [0, 1].  B = the sum over the slices with V_i = 0 of (T(t_i) - T(t_{i+1})), ascending i in
//              FP32 from 0, clamped to [0, A].  p = (1 - g g) / (q sqrtf(q)), q = (1 + g g) - (2 g) c, c = dot3(d, sun^), g = anisotropy,
//              sun^ normalised in FP64 by the host.  S_k = albedo_k ((sun_color_k p) (A - B) + ambient_color_k A).  A pixel without
//              kRayHit: A and S are multiplied by sky_affect.  color_k = color_k (1 - A) + S_k; a channel that is not finite takes S_k.
//              Writing the shadowed share as something SUBTRACTED is deliberate: a lit slice contributes exactly nothing, so a pixel
//              with no shadowed slice is the closed form to the bit; a NULL map, an empty map and a map whose casters no ray passes behind
//              give the same bytes; and a kernel may skip lit slices any way it likes (mist_span below) without changing a bit.
//   status     every pixel that is processed gets kRayMist; a pixel that carries it already is left alone (applying twice is applying
//              once).  Nothing but color and status changes.  A camera that is not finite (mesh_camera_ok) changes nothing.
//   out of scope: local fog volumes, density textures, temporal reprojection, light from the sky in the mist.  Spray drawn afterwards is not
//              fogged, as under ow_environment.h.
#pragma once

#include <cmath>

#include "ow_environment.h"
#include "ow_shadow.h"

namespace ow {

// layout-identical to ow_mist_options in include/ocean_waves.h
struct MistOptions {
    float extinction, height_falloff, base_height, length, anisotropy, sky_affect;
    int32_t slices;
    uint32_t flags;
    float shadow_bias;
    float albedo[3], sun_color[3], sun_direction[3], ambient_color[3];
    uint32_t reserved[11];
};
static_assert(sizeof(MistOptions) == 128 && offsetof(MistOptions, slices) == 24 && offsetof(MistOptions, shadow_bias) == 32 &&
                  offsetof(MistOptions, albedo) == 36 && offsetof(MistOptions, reserved) == 84,
              "record layout");

constexpr int32_t kRayMist = 256;               // OW_RAY_MIST
constexpr int kMistMaxSlices = 256;             // OW_MIST_MAX_SLICES
constexpr int kMistDefaultSlices = 64;
constexpr float kMistExtinctionMax = 1.0e3f, kMistFalloffMax = 1.0e3f, kMistAnisotropyMax = 0.9f;
constexpr float kMistRangeMax = 1.0e6f;         // |base_height|, length and |shadow_bias|
constexpr float kMistColorMax = 1.0e6f;         // the colours' channels, in [0, 1e6]
enum : int { kMistPixels = 0, kMistFetched = 1, kMistShadowed = 2, kMistCounters = 3 };
// The counters of a pass are kept in kMistCounterSlots copies, each on a 128-byte line of its own (kMistCounterStride 64-bit words apart):
// a wave adds to the copy of its block index, so the atomics of 14 400 waves do not queue on one address; the host sums the copies.
constexpr int kMistCounterSlots = 64, kMistCounterStride = 16;
constexpr size_t kMistCounterBytes = (size_t)kMistCounterSlots * kMistCounterStride * sizeof(unsigned long long);

// a pass's constants, resolved once from the options
struct MistParams {
    int camera_ok;       // 0: the camera is not finite -- nothing changes
    int slices;          // 1 .. kMistMaxSlices
    float extinction, k, base, length, g, sky_affect, bias;
    float albedo[3], sun_color[3], sun[3], ambient[3];
};

// Host code (FP64, a square root): the pass's constants from options the entry points have checked.  ok = false for a sun without a direction.
inline bool mist_params(const MistOptions &o, bool camera_ok, MistParams *mp) {
    __builtin_memset(mp, 0, sizeof(*mp));
    const double lx = o.sun_direction[0], ly = o.sun_direction[1], lz = o.sun_direction[2];
    const double len = sqrt(lx * lx + ly * ly + lz * lz);
    if (!(len > 0.0)) return false;
    mp->camera_ok = camera_ok ? 1 : 0;
    mp->slices = o.slices == 0 ? kMistDefaultSlices : o.slices;
    mp->extinction = o.extinction;
    mp->k = (float)((double)o.height_falloff * 0.69314718055994530942);
    mp->base = o.base_height;
    mp->length = o.length;
    mp->g = o.anisotropy;
    mp->sky_affect = o.sky_affect;
    mp->bias = o.shadow_bias;
    for (int k = 0; k < 3; ++k) {
        mp->albedo[k] = o.albedo[k];
        mp->sun_color[k] = o.sun_color[k];
        mp->sun[k] = (float)((double)o.sun_direction[k] / len);
        mp->ambient[k] = o.ambient_color[k];
    }
    return true;
}

// phi(x) = (1 - e^-x) / x for x >= 0; 1 at 0 and for a NaN
OW_DEV float mist_phi(float x) {
    if (!(x >= 0.5f)) {
        float p = 2.75573192e-6f;      // 1 / 9!
        p = 2.48015873e-5f - p * x;    // 1 / 8!
        p = 1.98412698e-4f - p * x;
        p = 1.38888889e-3f - p * x;
        p = 8.33333333e-3f - p * x;
        p = 4.16666667e-2f - p * x;
        p = 1.66666667e-1f - p * x;
        p = 0.5f - p * x;
        p = 1.0f - p * x;
        return x > 0.0f ? p : 1.0f;
    }
    return (1.0f - exp_f32(-x)) / x;
}

// I(t): h0 = o.y - base_height, dy = d.y, t >= 0
OW_DEV float mist_integral(float k, float h0, float dy, float t) {
    if (!(t > 0.0f)) return 0.0f;
    const float h1 = h0 + t * dy;
    if (h0 <= 0.0f && h1 <= 0.0f) return t;
    if (h0 >= 0.0f && h1 >= 0.0f) {
        const float lo = fminf(h0, h1), hi = fmaxf(h0, h1);
        return t * (exp_f32(-(k * lo)) * mist_phi(k * (hi - lo)));
    }
    float tc = -h0 / dy;                      // the signs differ, so dy is not 0
    tc = tc > 0.0f ? (tc < t ? tc : t) : 0.0f;
    const float below = h0 < 0.0f ? tc : t - tc, above = h0 < 0.0f ? t - tc : tc;
    return below + above * mist_phi(k * fmaxf(h0, h1));
}
OW_DEV float mist_transmittance(const MistParams &mp, float h0, float dy, float t) { return exp_f32(-(mp.extinction * mist_integral(mp.k, h0, dy, t))); }

OW_DEV float mist_phase(float g, float c) {
    const float g2 = g * g;
    const float q = (1.0f + g2) - (2.0f * g) * c;
    return (1.0f - g2) / (q * sqrtf(q));
}

OW_DEV float mist_boundary(float t_end, int i, int n) {
    const float f = (float)i / (float)n;
    return t_end * (f * f);
}

// One depth compare.  fetched: the map was read (the point lies in the footprint, within 2 depth_range, and is finite).
OW_DEV bool mist_lit(const ShadowParams &P, const uint32_t *map, float bias_m, const float w[3], bool &fetched) {
    fetched = false;
    float s, t, d;
    shadow_project(P, w, s, t, d);
    if (!(mesh_finite(s) && mesh_finite(t) && mesh_finite(d))) return true;
    const float side = (float)P.size;
    if (!(s >= 0.0f && s < side && t >= 0.0f && t < side) || d > P.max_depth) return true;
    fetched = true;
    return d - bias_m <= __builtin_bit_cast(float, map[(size_t)(int)t * P.size + (int)s]);
}

// The parameters m in [0, t_end] whose points can lie inside the frame's box (lo > hi: none), for a kernel that skips the others: outside
// the box mist_lit is true without a fetch.  (s, t, d) are affine in m up to rounding; the per-slice value rounds o_k + m d_k and then
// the difference from center_k (each within an ulp of |o|_1 + |center|_1 + t_end = reach), so it and this line are both within 1e-6 M
// of the exact one, M = k reach + size / 2 texels; the box is widened by 1 + 1e-5 M texels on each side, likewise in depth, so no slice
// that would fetch is ever skipped (tests/test_mist.py holds the two to the same bytes on fuzzed frames).  Anything not finite: the whole ray.
struct MistSpan {
    float lo, hi;
};
OW_DEV void mist_slab(float v0, float dv, float lo_v, float hi_v, MistSpan &sp) {
    if (dv == 0.0f) {
        if (!(v0 >= lo_v && v0 <= hi_v)) sp.hi = -1.0f, sp.lo = 0.0f;
        return;
    }
    const float a = (lo_v - v0) / dv, b = (hi_v - v0) / dv;
    sp.lo = fmaxf(sp.lo, fminf(a, b));
    sp.hi = fminf(sp.hi, fmaxf(a, b));
}
OW_DEV MistSpan mist_span(const ShadowParams &P, const float o[3], const float d[3], float t_end) {
    MistSpan sp = {0.0f, t_end};
    float r[3];
    float reach = t_end;   // the magnitudes whose roundings the per-slice point o + m d - center carries
    for (int k = 0; k < 3; ++k) {
        r[k] = o[k] - P.center[k];
        reach += fabsf(o[k]) + fabsf(P.center[k]);
    }
    const float s0 = dot3(P.x, r) * P.k + P.half, ds = dot3(P.x, d) * P.k;
    const float t0 = dot3(P.y, r) * P.k + P.half, dt = dot3(P.y, d) * P.k;
    const float d0 = P.depth_range - dot3(P.z, r), dd = -dot3(P.z, d);
    const float pad = 1.0f + 1.0e-5f * (P.k * reach + P.half), pad_d = 1.0e-3f + 1.0e-5f * (reach + P.depth_range);
    if (!(mesh_finite(pad) && mesh_finite(s0) && mesh_finite(t0) && mesh_finite(d0) && mesh_finite(ds) && mesh_finite(dt))) return sp;
    const float side = (float)P.size;
    mist_slab(s0, ds, -pad, side + pad, sp);
    mist_slab(t0, dt, -pad, side + pad, sp);
    const float far = P.max_depth + pad_d;
    if (dd == 0.0f) {
        if (d0 > far) sp.hi = -1.0f, sp.lo = 0.0f;
    } else {
        const float m = (far - d0) / dd;
        if (dd > 0.0f)
            sp.hi = fminf(sp.hi, m);
        else
            sp.lo = fmaxf(sp.lo, m);
    }
    if (!(sp.lo == sp.lo && sp.hi == sp.hi)) return MistSpan{0.0f, t_end};   // a NaN (none can arise: no 0 / 0, no Inf - Inf): the whole ray
    return sp;
}

// what the pass makes of one pixel, with the intermediates the tests read
struct MistPixel {
    bool changed;       // color and status are to be written
    int32_t status;
    float color[3];
    float A, B;         // before sky_affect
    float S[3];         // after it
    uint32_t fetched, shadowed;   // slices whose compare read the map; slices with V = 0
};
// map: the depth words, or null (no map, or one without a frame: P is not read then).  skip: leave out the slices outside mist_span.
OW_DEV MistPixel mist_pixel(const MistParams &mp, const ShadowParams &P, const uint32_t *map, const CameraParams &cam, int i, int j, float t, int32_t status,
                            const float color[3], bool skip) {
    MistPixel px;
    px.changed = false;
    px.status = status;
    px.A = px.B = 0.0f;
    px.fetched = px.shadowed = 0u;
    for (int k = 0; k < 3; ++k) {
        px.color[k] = color[k];
        px.S[k] = 0.0f;
    }
    if (!mp.camera_ok || (status & kRayMist)) return px;
    px.changed = true;
    px.status = status | kRayMist;
    float d[3];
    env_ray(cam, i, j, d);
    const bool hit = (status & kRayHit) != 0;
    const float t_end = hit ? (t > 0.0f ? fminf(t, mp.length) : 0.0f) : mp.length;
    const float h0 = cam.o[1] - mp.base, dy = d[1];
    float A = 1.0f - mist_transmittance(mp, h0, dy, t_end);
    A = env_clamp01(A);
    float B = 0.0f;
    if (map) {
        const float bias_m = mp.bias * P.w;
        MistSpan sp = {0.0f, t_end};
        if (skip) sp = mist_span(P, cam.o, d, t_end);
        for (int n = 0; n < mp.slices; ++n) {      // the same trip count for every pixel
            const float ta = mist_boundary(t_end, n, mp.slices), tb = mist_boundary(t_end, n + 1, mp.slices);
            const float m = 0.5f * (ta + tb);
            if (!(m >= sp.lo && m <= sp.hi)) continue;
            float w[3];
            for (int k = 0; k < 3; ++k) w[k] = cam.o[k] + m * d[k];
            bool fetched;
            const bool lit = mist_lit(P, map, bias_m, w, fetched);
            px.fetched += fetched ? 1u : 0u;
            if (lit) continue;
            ++px.shadowed;
            B = B + (mist_transmittance(mp, h0, dy, ta) - mist_transmittance(mp, h0, dy, tb));
        }
        B = B > 0.0f ? (B < A ? B : A) : 0.0f;
    }
    px.A = A;
    px.B = B;
    const float p = mist_phase(mp.g, dot3(d, mp.sun));
    float S[3];
    for (int k = 0; k < 3; ++k) S[k] = mp.albedo[k] * ((mp.sun_color[k] * p) * (A - B) + mp.ambient[k] * A);
    if (!hit) {
        A = A * mp.sky_affect;
        for (int k = 0; k < 3; ++k) S[k] = S[k] * mp.sky_affect;
    }
    for (int k = 0; k < 3; ++k) {
        const float v = color[k] * (1.0f - A) + S[k];
        px.S[k] = S[k];
        px.color[k] = mesh_finite(v) ? v : S[k];
    }
    return px;
}

}  // namespace ow

// ow_mirror.h -- the floating bodies' image in the water (include/ocean_waves.h ow_mirror_*): the sky-light pass of ow_sky_light.h with one
// thing added.  Where a water pixel's mirror ray meets a body at its resident pose, the pixel reflects that body's lit colour instead of the
// sky pyramid.  The pass takes ow_radiance_light_apply's place in the frame order:
//     water -> solids -> ow_shadow_apply -> ow_mirror_apply -> ow_environment_apply -> ow_mist_apply -> billboards -> ow_present
//
// Compiles as device code (ow_mirror.hip, built with -ffp-contract=off) and as plain C++ (tests/mirror/, g++ -ffp-contract=off), like
// ow_sky_light.h and ow_solid_cast.h, whose functions it calls: both builds produce the same bits for every input.  THIS LIBRARY'S CHOICE
// throughout: the engine's screen-space reflections are not part of the reference, so this header is the authority.
//
//   records    sky_light_pixel's conditions exactly (sky_light_begin): a record WITH kRayHit and WITHOUT kRayEnvironment and kRaySkyLit is
//              processed and gets kRaySkyLit; only color and status change; a camera that is not finite changes nothing; twice is once;
//              after ow_radiance_light_apply, nothing.
//   sky        view, ambient, reflect, lod, radiance and env are sky_light_begin's; spec and color are sky_light_finish's.  Where no body
//              is met the record is ow_radiance_light_apply's to the bit.
//   ray        only for water seen from above (sky_light_begin returns kSkyLightWater) and only when there is at least one instance: an
//              ow_ray with origin = position, direction = reflect (the FP32 values of the sky pass), max_distance = the options'.  Such a
//              record CASTS.
//   hit        ow_solid_cast.h's to the bit: ray_setup without a slab, solid_cast_pair over every pair of every instance that is not
//              skipped, the smallest word (bits of t << 32) | pair; T = max_distance: there is no water limit.  One-sided unless
//              kMirrorTwoSided: a ray that starts inside a half-sunk crate sees nothing.  A ray that ray_setup calls invalid meets nothing
//              (its hit record is the cast's: zeros with kRayInvalid).
//   on a hit   h = solid_cast_record's record, n = h.normal, t = h.t.  If n is zero (solid_cast_record stores zeros for a normal that is
//              not finite) nothing more happens.  Otherwise, per channel k and in this order in FP32:
//                ndl  = fmaxf(dot3(n, l), 0)                                     l: the unit vector towards the light (FP64 on the host)
//                e    = tap(E, n)                                                 radiance_tap of the irradiance texture
//                C_k  = body_color_k * ((light_color_k * ndl + ambient_color_k) + e_k * ambient_energy)
//                fade = t <= fade_begin ? 1 : (max_distance - t) / (max_distance - fade_begin)
//                w    = opacity * fade
//                radiance'_k = glsl_mix(radiance_k, C_k, w) = radiance_k (1 - w) + C_k w
//              The draw's terms (ow_solid.h solid_pixel) plus the sky ambient the body itself receives, unshadowed.  If a C_k is not finite
//              radiance stays as it was.  Otherwise radiance' replaces radiance, the record gets kRayMirror, and sky_light_finish runs on it.
//   hits       the optional output: for a record that casts, what ow_cast_bodies writes for its ray; for every other record the no-hit
//              record (status 0, instance = triangle = -1, the rest 0).
//   culling    is no part of the definition.  A ray goes on to an instance's triangles when solid_cast_sphere_pass says so.  Ahead of that the
//              kernel drops, for a whole 8 x 8 tile at once, the instances no ray of the tile can pass (mirror_bundle_pass below): with the
//              tile's rays o + t d^ bounded per axis by [omin + t dmin, omax + t dmax], a ray that passes the sphere test has a point at
//              some 0 <= t <= T within sqrt(2) of the test's inflated radius of the centre (the test lets a sphere through whose nearest
//              point lies up to a radius behind the origin or beyond T), so per axis |o_k + t d^_k - c_k| <= 1.5 r + margin for one t:
//              six linear inequalities in t, intersected with [0, 1.001 T].  What it drops no lane's sphere test would pass, so neither
//              the records nor the counters depend on it; the CPU build checks that claim instance by instance (tests/mirror/).
//   counters   pixels processed, rays cast, sphere tests passed (instances that went on to their triangles: with culling off every
//              instance that is not skipped), pairs tested, rays that hit.
//   not here   the water reflected in itself; shadows on the mirrored body; roughness blur of the mirrored image (the body's image is
//              sharp whatever the water's roughness; only the sky's is blurred); reflections in the spray; a group form.
#pragma once

#include "ow_sky_light.h"
#include "ow_solid_cast.h"

namespace ow {

// layout-identical to ow_mirror_options in include/ocean_waves.h
struct MirrorOptions {
    float ambient_energy, reflection_energy, specular;
    float body_color[3];
    float light_direction[3];
    float light_color[3];
    float ambient_color[3];
    float max_distance, fade_begin, opacity;
    uint32_t flags;
    int32_t cull;
    uint32_t reserved[12];
};
static_assert(sizeof(MirrorOptions) == 128 && offsetof(MirrorOptions, body_color) == 12 && offsetof(MirrorOptions, max_distance) == 60 &&
                  offsetof(MirrorOptions, flags) == 72 && offsetof(MirrorOptions, reserved) == 80,
              "record layout");

constexpr int32_t kRayMirror = 512;          // OW_RAY_MIRROR
constexpr uint32_t kMirrorTwoSided = 1u;     // OW_MIRROR_TWO_SIDED
constexpr float kMirrorDistanceMax = 1.0e12f;
constexpr float kMirrorDefaultDistance = 200.0f, kMirrorDefaultFadeBegin = 100.0f;

// the five counters of a pass
enum : int { kMirrorPixels = 0, kMirrorRays = 1, kMirrorPassed = 2, kMirrorPairs = 3, kMirrorHits = 4, kMirrorCounters = 5 };

// a pass's constants beyond the sky pass's, resolved once from the options
struct MirrorParams {
    float body_color[3];
    float light[3];  // the unit vector towards the light (normalised in FP64 on the host)
    float light_color[3], ambient_color[3];
    float max_distance, fade_begin, opacity;
    SolidCastParams cp;  // two_sided, cull
};

// what the pass makes of one record; the tests read the intermediates
struct MirrorPixel {
    SkyLightPixel sky;  // sky_light_pixel's, radiance being radiance' where a body is mirrored
    int stage;          // sky_light_begin's
    bool cast;
    RaySetup s;         // of the mirror ray (cast only)
    float body[3];      // C (zeros without a hit)
    float weight;       // w
};

// the first part: the sky pass up to radiance, and the mirror ray's set-up where the record casts
OW_DEV void mirror_begin(const SkyLightParams &lp, const MirrorParams &mp, int instances, const CameraParams &cam, int i, int j, int32_t status,
                         const float position[3], const float albedo[3], const float normal[3], float roughness, const float color[3], MirrorPixel &px) {
    px.stage = sky_light_begin(lp, cam, i, j, status, position, albedo, normal, roughness, color, px.sky);
    px.cast = px.stage == kSkyLightWater && instances > 0;
    px.body[0] = px.body[1] = px.body[2] = px.weight = 0.0f;
    Ray ray;
    for (int k = 0; k < 3; ++k) {
        ray.origin[k] = px.cast ? position[k] : 0.0f;
        ray.direction[k] = px.cast ? px.sky.reflect[k] : 0.0f;
    }
    ray.max_distance = mp.max_distance;
    ray.reserved = 0u;
    px.s = ray_setup(ray, kSolidCastNoSlab, 0.0f);  // not valid where the record does not cast
}

// ---- the tile's bundle of rays ----
// the box of the origins and of the unit directions of a tile's searching rays, and what the test below needs of them
struct MirrorBundle {
    float omin[3], omax[3], dmin[3], dmax[3];
    float omag;  // the sum over the axes of the largest |origin component|
    float T;     // 1.001 max_distance
};
OW_DEV void mirror_bundle_empty(MirrorBundle &B) {
    for (int k = 0; k < 3; ++k) {
        B.omin[k] = B.dmin[k] = 3.4028235e38f;
        B.omax[k] = B.dmax[k] = -3.4028235e38f;
    }
    B.omag = B.T = 0.0f;
}
// one searching ray into the bundle (the kernel does the same with wave reductions)
OW_DEV void mirror_bundle_add(MirrorBundle &B, const RaySetup &s) {
    for (int k = 0; k < 3; ++k) {
        B.omin[k] = s.o[k] < B.omin[k] ? s.o[k] : B.omin[k];
        B.omax[k] = s.o[k] > B.omax[k] ? s.o[k] : B.omax[k];
        B.dmin[k] = s.d[k] < B.dmin[k] ? s.d[k] : B.dmin[k];
        B.dmax[k] = s.d[k] > B.dmax[k] ? s.d[k] : B.dmax[k];
    }
}
OW_DEV void mirror_bundle_close(MirrorBundle &B, float max_distance) {
    B.omag = 0.0f;
    for (int k = 0; k < 3; ++k) {
        const float a = fabsf(B.omin[k]), b = fabsf(B.omax[k]);
        B.omag += a > b ? a : b;
    }
    B.T = max_distance * 1.001f;
}
// Can a ray of the bundle pass solid_cast_sphere_pass for this sphere?  False only where none can; every comparison is written so that a
// NaN or an Inf passes.  The margin: the sphere test inflates r by 2^-21 (|c - o| + r) and by slacks of 1e-7 |c - o|, well under
// 1e-5 (|c| + |o| + r); the quotients' own rounding is covered by widening each bound by 1e-5 of itself.
OW_DEV bool mirror_bundle_pass(const MirrorBundle &B, const SolidCastBound &b) {
    if (b.r < 0.0f) return false;  // skipped
    const float cmag = (fabsf(b.c[0]) + fabsf(b.c[1])) + fabsf(b.c[2]);
    const float pad = 1.5f * b.r + (1e-5f * ((cmag + B.omag) + b.r) + 1e-30f);
    float lo = 0.0f, hi = B.T;
    for (int k = 0; k < 3; ++k) {
        const float a = (b.c[k] - B.omax[k]) - pad;  // a <= t dmax
        const float e = (b.c[k] - B.omin[k]) + pad;  // t dmin <= e
        if (B.dmax[k] > 0.0f) {
            float q = a / B.dmax[k];
            q -= 1e-5f * fabsf(q);
            lo = q > lo ? q : lo;
        } else if (B.dmax[k] < 0.0f) {
            float q = a / B.dmax[k];
            q += 1e-5f * fabsf(q);
            hi = q < hi ? q : hi;
        } else if (a > 0.0f) {
            return false;
        }
        if (B.dmin[k] > 0.0f) {
            float q = e / B.dmin[k];
            q += 1e-5f * fabsf(q);
            hi = q < hi ? q : hi;
        } else if (B.dmin[k] < 0.0f) {
            float q = e / B.dmin[k];
            q -= 1e-5f * fabsf(q);
            lo = q > lo ? q : lo;
        } else if (e < 0.0f) {
            return false;
        }
    }
    return !(lo > hi);
}

// One lane's search for its own ray over every instance: the straightforward form, which the CPU build runs.  bounds: the instances' spheres
// (solid_cast_instance_bound; radius < 0: skipped).  passed, pairs: added to.
OW_DEV uint64_t mirror_search_lane(const SolidCastShape &shape, const SolidInstances &in, const SolidCastBound *bounds, const SolidCastParams &cp,
                                   const RaySetup &s, float T, uint32_t &passed, uint32_t &pairs) {
    uint64_t best = kSolidCastNoHit;
    const int nt = shape.num_triangles;
    for (int inst = 0; inst < in.count; ++inst) {
        const SolidCastBound b = bounds[inst];
        if (!(cp.cull ? solid_cast_sphere_pass(b, s, T) : !(b.r < 0.0f))) continue;
        ++passed;
        pairs += (uint32_t)nt;
        const float *tf = solid_transform(in, inst);
        for (int tri = 0; tri < nt; ++tri) {
            const SolidCastPair pr = solid_cast_pair(shape, tf, s, T, cp.two_sided, tri);
            if (!pr.hit) continue;
            const uint64_t word = solid_cast_word(pr.t, inst * nt + tri);
            best = word < best ? word : best;
        }
    }
    return best;
}

// the record of hits_out: ow_cast_bodies' for a record that casts, the no-hit record otherwise
OW_DEV SolidHit mirror_hit_record(const SolidCastShape &shape, const SolidInstances &in, const MirrorParams &mp, const MirrorPixel &px, uint64_t word) {
    if (!px.cast) return solid_cast_record(shape, in, px.s, mp.max_distance, mp.cp.two_sided, kSolidCastNoHit);
    SolidCastWinner win;
    win.s = px.s;
    win.T = mp.max_distance;
    win.word = px.s.valid ? word : kSolidCastNoHit;
    return solid_cast_finish(shape, in, mp.cp, win);
}

// the second part: the body's colour into radiance where h is a hit, then the rest of the sky pass.  Returns whether the record is mirrored.
OW_DEV bool mirror_finish(const SkyLightParams &lp, const MirrorParams &mp, const float color[3], const SolidHit &h, MirrorPixel &px) {
    bool mirrored = false;
    if (px.cast && (h.status & kRayHit)) {
        const float *n = h.normal;
        if (!(n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f)) {
            const float ndl = fmaxf(dot3(n, mp.light), 0.0f);
            float e[3];
            radiance_tap(lp.E, n, e);
            bool ok = true;
            for (int k = 0; k < 3; ++k) {
                px.body[k] = mp.body_color[k] * ((mp.light_color[k] * ndl + mp.ambient_color[k]) + e[k] * lp.ambient_energy);
                ok = ok && mesh_finite(px.body[k]);
            }
            if (ok) {
                const float fade = h.t <= mp.fade_begin ? 1.0f : (mp.max_distance - h.t) / (mp.max_distance - mp.fade_begin);
                px.weight = mp.opacity * fade;
                for (int k = 0; k < 3; ++k) px.sky.radiance[k] = glsl_mix(px.sky.radiance[k], px.body[k], px.weight);
                px.sky.status |= kRayMirror;
                mirrored = true;
            }
        }
    }
    sky_light_finish(lp, color, px.stage, px.sky);
    return mirrored;
}

}  // namespace ow

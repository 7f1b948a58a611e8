// ow_raycast.h -- ray casts against the rendered water surface (include/ocean_waves.h ow_raycast_surface): where a ray first meets the
// height field the water-height query reports.
//
// Compiles as device code (ow_consumer.hip, built with -ffp-contract=off) and as plain C++ (tests/raycast/, g++ -ffp-contract=off), like
// ow_surface.h and ow_buoyancy.h: every operation is an IEEE-754 FP32 add, multiply, divide, square root, min / max or compare, or integer
// work on the FP16 bits, so both builds produce the same bits.  The kernel runs one 64-lane wave per ray; the CPU build runs the same
// round logic (raycast_ray below) with the 64 lanes stepped one after the other (SerialWave).
//
// The water is the height field h(x, z) = ow_surface_query.height at (x, z): a cold query_solve from q = (x, z), then f(p) * D_y(p)
// (displacement_y: the same bits as the query's height).  For a ray with origin o, direction d and max_distance T:
//   d^ = d / sqrt((dx dx + dy dy) + dz dz)        t is metres along d^
//   g(t) = (o.y + t d^.y) - (water_level + h(o.x + t d^.x, o.z + t d^.z))       g > 0: the ray point is above the water
// The hit is the first t in [0, T] whose sign class (g > 0 or not) differs from the class at the first sample:
//   1. Slab.  H = sum_c maxabs_c * |s_z,c| in cascade order (maxabs_c: the largest |D_y| over layer c's texels, taken as the max of the
//      FP16 magnitude bits and converted once), widened to Hw = H * (1 + 2^-10) + kSlabFloor.  |h| <= Hw everywhere: each cascade's
//      bilinear interpolant of values within [-maxabs, maxabs] has weights in [0, 1] that sum to 1, so its FP32 evaluation exceeds
//      maxabs by a few ulp at most; the scale, the sum over at most 8 cascades and the falloff f <= 1 (exp_f32 within a few ulp) add a
//      few ulp each -- some 2^-20 relative in all, well inside 2^-10.  The floor keeps a calm sea (H = 0) bracketing the plane.  A
//      non-finite Hw makes the slab the whole ray.  The ray can cross the water only where |o.y + t d^.y - water_level| <= Hw: that
//      interval, intersected with [0, T], is [t_in, t_out].  A ray that never enters it evaluates no sample and has no hit.
//   2. March.  t_k = min(t_in + (float)k * spacing, t_out) for k = 0, 1, ..., up to the first k with t_in + k * spacing >= t_out, in
//      rounds of 64 (round r: k = 64 r .. 64 r + 63, lane j takes k = 64 r + j).  The first k >= 1 whose class differs from t_0's gives
//      the bracket [t_(k-1), t_k].  If max_samples runs out before t_out, the ray is TRUNCATED.
//   3. Refine.  a + (b - a) * ((float)j * 0.015625f) for j = 1 .. 63 (lane j), with b as the 64th point; the first class change is the
//      new bracket.  Repeated while b - a > tolerance, at most kRefineRounds times; then t = a + (b - a) * (g_a / (g_a - g_b)), clamped
//      into [a, b].
//   4. Record.  position = o + t d^ per component; query_point at (position.x, position.z) is embedded, and residual = position.y -
//      (water_level + query.height) is g(t) exactly.
// Sampling limits: a crest narrower than the sample spacing, measured along the ray, can be missed (both crossings of a thin crest
// may fall between two samples), and so can a crossing inside the last few ulp of the slab at very large t.  Folded crests have no
// height field: h there is the query's best iterate, and the embedded record's converged flag says so.
#pragma once

#include "ow_buoyancy.h"

namespace ow {

// layout-identical to ow_ray / ow_raycast_hit in include/ocean_waves.h
struct Ray {
    float origin[3];
    float max_distance;
    float direction[3];
    uint32_t reserved;
};
struct RaycastHit {
    float t;
    float position[3];
    float residual;
    int32_t status;
    int32_t samples;  // evaluations of g
    int32_t rounds;   // 64-lane rounds: march and refine
    float slab_half_height, t_enter, t_exit;
    uint32_t reserved[5];
    SurfaceQuery query;
};
static_assert(sizeof(Ray) == 32 && sizeof(RaycastHit) == 192 && offsetof(RaycastHit, query) == 64, "record layout");

// the status bits (OW_RAY_* in include/ocean_waves.h)
constexpr int32_t kRayHit = 1;        // the ray meets the water at t
constexpr int32_t kRayFromBelow = 2;  // its first sample (or, outside the slab, its origin) is not above the water: a hit leaves it
constexpr int32_t kRayTruncated = 4;  // max_samples ran out before t_out without a bracket
constexpr int32_t kRayInvalid = 8;    // non-finite origin, direction or max_distance, max_distance <= 0, or a zero-length direction

// The defaults.  0.25 m spacing: one round of 64 samples covers 16 m of ray, which holds the whole slab of the demo scene (Hw about
// 2-3 m) for rays steeper than about 20 degrees, so such a ray brackets in one round; a crest must be narrower than 0.25 m along the ray
// to be missed, a few texels of the finest demo cascade (88 m over 1024 texels).  4096 samples: 1 km of ray at that spacing, 64 rounds.
constexpr float kRayDefaultSpacing = 0.25f;
constexpr float kRayDefaultTolerance = 1e-3f;
constexpr int kRayDefaultMaxSamples = 4096;
constexpr int kRayMaxSamples = 1 << 20;
constexpr int kRefineRounds = 4;      // 64^4 = 2^24: from any spacing <= 1 m to FP32 resolution
constexpr float kSlabFloor = 1e-2f;   // metres: the slab's absolute floor
struct RaycastParams {
    QueryParams qp;     // the height solve
    float water_level;  // metres
    float spacing;      // metres along the ray, > 0
    float tolerance;    // metres along the ray, > 0
    int max_samples;    // 1 .. kRayMaxSamples
};

// |D_y| of one texel as FP16 magnitude bits: the sign cleared; a max over these, converted once, is the exact largest |D_y|
OW_DEV uint32_t dy_magnitude_bits(const u16x4 &t) { return (uint32_t)(t.y & 0x7fffu); }

// Hw from the per-cascade magnitude bits (step 1); FLT_MAX stands for "the whole ray" (a non-finite bound)
OW_DEV float slab_half_height(const uint32_t *bits, int cascades, const SurfaceScales &scales) {
    float H = 0.0f;
    for (int c = 0; c < cascades; ++c) H += h2f((uint16_t)bits[c]) * fabsf(scales.s[c][2]);
    const float hw = H * (1.0f + 0.0009765625f) + kSlabFloor;
    return finite_f32(hw) ? hw : 3.4028235e38f;
}

// a ray after normalisation and the slab (wave-uniform)
struct RaySetup {
    float o[3], d[3];  // origin, d^
    float t_in, t_out;
    bool valid, enters, below;  // below: the origin lies under the slab (only read when the ray does not enter it)
};

OW_DEV RaySetup ray_setup(const Ray &ray, float hw, float water_level) {
    RaySetup s;
    bool ok = finite_f32(ray.max_distance) && ray.max_distance > 0.0f;
    for (int k = 0; k < 3; ++k) ok = ok && finite_f32(ray.origin[k]) && finite_f32(ray.direction[k]);
    const float len = ok ? sqrtf((ray.direction[0] * ray.direction[0] + ray.direction[1] * ray.direction[1]) + ray.direction[2] * ray.direction[2])
                         : 0.0f;
    s.valid = ok && len > 0.0f && finite_f32(len);  // a squared length that underflows to 0 or overflows counts as zero-length
    s.enters = s.below = false;
    s.t_in = s.t_out = 0.0f;
    for (int k = 0; k < 3; ++k) {
        s.o[k] = s.valid ? ray.origin[k] : 0.0f;
        s.d[k] = s.valid ? ray.direction[k] / len : 0.0f;
    }
    if (!s.valid) return s;
    const float T = ray.max_distance, rel = s.o[1] - water_level;
    float lo = 0.0f, hi = T;
    if (hw >= 3.4028235e38f) {
        s.enters = true;  // no bound: the whole ray
    } else if (s.d[1] == 0.0f) {
        s.enters = fabsf(rel) <= hw;
    } else {
        const float t1 = ((water_level + hw) - s.o[1]) / s.d[1], t2 = ((water_level - hw) - s.o[1]) / s.d[1];
        const float a = t1 < t2 ? t1 : t2, b = t1 < t2 ? t2 : t1;
        lo = a > 0.0f ? a : 0.0f;
        hi = b < T ? b : T;
        s.enters = lo <= hi;
    }
    s.below = rel < -hw;
    if (s.enters) {
        s.t_in = lo;
        s.t_out = hi;
    }
    return s;
}

// one sample: g at t and the height h it saw
struct RaySample {
    float t, g, h;
};
OW_DEV RaySample ray_sample(const u16x4 *disp, int n, int cascades, const SurfaceScales &scales, const RaycastParams &rp, const RaySetup &s,
                            float t) {
    const float x = s.o[0] + t * s.d[0], y = s.o[1] + t * s.d[1], z = s.o[2] + t * s.d[2];
    const QuerySolution sol = query_solve(disp, n, cascades, scales, rp.qp, x, z, x, z);
    RaySample r;
    r.t = t;
    r.h = sol.e.f * displacement_y(disp, n, cascades, scales, sol.p[0], sol.p[1]);
    r.g = y - (rp.water_level + r.h);
    return r;
}

// the t of lane j in march round r, and whether the lane takes a sample (in range and within max_samples) or was cut by max_samples
OW_DEV float march_t(const RaySetup &s, float spacing, int k) {
    const float t = s.t_in + (float)k * spacing;
    return t < s.t_out ? t : s.t_out;
}
OW_DEV bool march_in_range(const RaySetup &s, float spacing, int k) { return k == 0 || s.t_in + (float)(k - 1) * spacing < s.t_out; }
OW_DEV float refine_t(float a, float b, int j) { return j >= 64 ? b : a + (b - a) * ((float)j * 0.015625f); }

OW_DEV int lowest_bit(uint64_t m) { return __builtin_ctzll(m); }
OW_DEV int bit_count(uint64_t m) { return __builtin_popcountll(m); }

OW_DEV RaycastHit ray_record_zero() {
    RaycastHit h;
    __builtin_memset(&h, 0, sizeof(h));
    return h;
}

// Steps 2-4 for one ray.  Wave is the 64 lanes: wave.round(pred, fn, took, above) has lane j evaluate fn(j) -> RaySample where pred(j)
// holds, and returns the ballots of the lanes that sampled (took) and of those whose sample lies above the water (above: g > 0);
// wave.t(j) / wave.g(j) read lane j's sample of the last round.  Everything here outside fn is wave-uniform.
template <class Wave>
OW_DEV RaycastHit raycast_ray(Wave &wave, const u16x4 *disp, const u16x4 *norm, int n, int cascades,
                              const SurfaceScales &scales, const RaycastParams &rp, const Ray &ray, float hw) {
    RaycastHit out = ray_record_zero();
    const RaySetup s = ray_setup(ray, hw, rp.water_level);
    if (!s.valid) {
        out.status = kRayInvalid;
        return out;
    }
    out.slab_half_height = hw;
    out.t_enter = s.t_in;
    out.t_exit = s.t_out;
    if (!s.enters) {
        out.status = s.below ? kRayFromBelow : 0;
        return out;
    }
    auto sample = [&](float t) { return ray_sample(disp, n, cascades, scales, rp, s, t); };
    // 2. march
    bool above0 = false, bracket = false, truncated = false;
    float a = 0.0f, b = 0.0f, ga = 0.0f, gb = 0.0f, t_last = 0.0f, g_last = 0.0f;
    for (int r = 0;; ++r) {
        const int kb = 64 * r;
        if (!march_in_range(s, rp.spacing, kb)) break;  // the previous round ended at t_out
        if (kb >= rp.max_samples) {
            truncated = true;
            break;
        }
        uint64_t took, above;
        wave.round([&](int j) { const int k = kb + j; return k < rp.max_samples && march_in_range(s, rp.spacing, k); },
                   [&](int j) { return sample(march_t(s, rp.spacing, kb + j)); }, took, above);
        ++out.rounds;
        out.samples += bit_count(took);
        if (r == 0) above0 = (above & 1u) != 0;
        uint64_t change = took & (above0 ? ~above : above);
        if (change) {
            const int j = lowest_bit(change);
            b = wave.t(j);
            gb = wave.g(j);
            if (j > 0) {
                a = wave.t(j - 1);
                ga = wave.g(j - 1);
            } else {
                a = t_last;
                ga = g_last;
            }
            bracket = true;
            break;
        }
        if (took != ~(uint64_t)0) {  // the round ended at t_out, or at max_samples
            truncated = kb + 64 > rp.max_samples && march_in_range(s, rp.spacing, rp.max_samples);
            break;
        }
        t_last = wave.t(63);
        g_last = wave.g(63);
    }
    out.status = above0 ? 0 : kRayFromBelow;
    if (!bracket) {
        if (truncated) out.status |= kRayTruncated;
        return out;
    }
    // 3. refine
    for (int i = 0; i < kRefineRounds && b - a > rp.tolerance; ++i) {
        const float ra = a, rb = b;
        uint64_t took, above;
        wave.round([&](int j) { return j >= 1; }, [&](int j) { return sample(refine_t(ra, rb, j)); }, took, above);
        ++out.rounds;
        out.samples += bit_count(took);
        const uint64_t change = took & (above0 ? ~above : above);
        if (change) {
            const int j = lowest_bit(change);
            b = wave.t(j);
            gb = wave.g(j);
            if (j > 1) {
                a = wave.t(j - 1);
                ga = wave.g(j - 1);
            }
        } else {  // the change lies between lane 63 and b
            a = wave.t(63);
            ga = wave.g(63);
        }
    }
    const float w = ga / (ga - gb);
    float t = a + (b - a) * w;
    t = t > a ? (t < b ? t : b) : a;  // NaN -> a
    // 4. record
    out.t = t;
    for (int k = 0; k < 3; ++k) out.position[k] = s.o[k] + t * s.d[k];
    out.query = query_point(disp, norm, n, cascades, scales, rp.qp, out.position[0], out.position[2]);
    out.residual = out.position[1] - (rp.water_level + out.query.height);
    out.status |= kRayHit;
    return out;
}

// The 64 lanes stepped one after the other (the CPU build).  max_abs_h: the largest |h| any sample saw (a test's probe).
struct SerialWave {
    float ts[64], gs[64];
    float max_abs_h = 0.0f;
    template <class Pred, class Fn>
    void round(const Pred &pred, const Fn &fn, uint64_t &took, uint64_t &above) {
        took = above = 0;
        for (int j = 0; j < 64; ++j) {
            ts[j] = gs[j] = 0.0f;
            if (!pred(j)) continue;
            const RaySample smp = fn(j);
            ts[j] = smp.t;
            gs[j] = smp.g;
            const float ah = fabsf(smp.h);
            if (!(ah <= max_abs_h)) max_abs_h = ah;
            took |= (uint64_t)1 << j;
            if (smp.g > 0.0f) above |= (uint64_t)1 << j;
        }
    }
    float t(int j) const { return ts[j]; }
    float g(int j) const { return gs[j]; }
};

}  // namespace ow

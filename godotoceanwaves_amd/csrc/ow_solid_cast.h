// ow_solid_cast.h -- ray casts against solids at instance transforms (include/ocean_waves.h ow_cast_*): where a ray first meets the
// floating bodies of ow_bodies_* (or a caller's transforms), as ow_raycast_surface says where it meets the water.
//
// Compiles as device code (ow_solid_cast.hip, built with -ffp-contract=off) and as plain C++ (tests/solid_cast/, g++ -ffp-contract=off), like
// ow_solid.h: every operation is an IEEE-754 add, subtract, multiply, divide, square root or compare, in FP32 or FP64, so both builds produce
// the same bits.  The kernel runs one 64-lane wave per ray; the CPU build runs the same functions (solid_cast_search and solid_cast_finish
// below) with the 64 lanes stepped one after the other (SolidCastSerialWave).
//
//   ray        ow_raycast.h's ray_setup with hw = 3.4028235e38f (no slab): validity and the unit direction d^ are its.  A ray that is not valid
//              gives the all-zero record with kRayInvalid.
//   instances  ow_solid.h's: instance i's twelve floats, skipped when solid_instance_ok says so.
//   vertices   solid_world's bits.  A triangle with a vertex that is not finite is skipped.
//   pair       (instance, triangle), numbered instance * num_triangles + triangle.  With p_k = w_k - o in FP32 (o: the ray's origin) and
//              everything after that in FP64:
//                N  = (p1 - p0) x (p2 - p0)
//                e0 = d^ . (p1 x p2), e1 = d^ . (p2 x p0), e2 = d^ . (p0 x p1)        a x b = (ay bz - az by, az bx - ax bz, ax by - ay bx),
//                dn = d^ . N                                                          u . v = (ux vx + uy vy) + uz vz
//              so that a x b = -(b x a) to the bit: two triangles that share an edge compute that edge's function with opposite sign and
//              equal magnitude (ow_mesh.h's plane vectors have the same property).  dn < 0 is the front (outward, counter-clockwise) side.
//              The ray meets the triangle when dn != 0 and none of e0, e1, e2 has the sign opposite to dn's (e0 + e1 + e2 = dn in exact
//              arithmetic: the e_i / dn are the hit's barycentrics, and the ray is inside where none is negative).  Zeros pass: edges are
//              inclusive, so a ray through a shared edge or vertex of a closed mesh is never lost.
//                t = (p0 . N) / dn, narrowed once to FP32, -0 stored as +0; the pair qualifies when 0 <= t <= T.
//   facing     back faces (dn > 0) are dropped unless the cast is two-sided; then they qualify and the reported normal is negated.
//   limit      T = max_distance; with the water's record for the ray (an ow_raycast_hit as ow_raycast_surface wrote it) that has kRayHit,
//              T = water.t where water.t < T.  The water is opaque, as in the draw's depth rule.
//   winner     of all qualifying pairs the smallest 64-bit word (bits of t << 32) | pair: whatever the launch shape, the order or the culling.
//   record     t; position = o + t d^ per component in FP32 (ow_raycast.h's order; an overflow is stored as +-FLT_MAX); normal = solid_normal
//              of the three world vertices (ow_solid.h), zeros if it is not finite; status = kRayHit | kRaySolid; instance, triangle;
//              barycentric = e1 / s, e2 / s with s = (e0 + e1) + e2, narrowed once (0, 0 if s is 0).  Without a hit: status 0, instance =
//              triangle = -1, everything else 0.  Nothing written is a NaN or an Inf.
//   culling    is no part of the definition.  Instances are culled by a bounding sphere: the shape's local centre and radius (solid_cast_shape_bound:
//              the middle of the finite vertices' box, the largest distance from it), the world centre by solid_world, the radius inflated by the
//              basis's Frobenius norm and a bound on the FP32 rounding of the world vertices (solid_cast_instance_bound), the ray-sphere test in
//              FP64 with the rounding of p_k = w_k - o added to the radius (solid_cast_sphere_pass).  Every comparison is written so that a NaN
//              or an Inf passes.  The records do not depend on it.
#pragma once

#include <cmath>

#include "ow_raycast.h"
#include "ow_solid.h"

namespace ow {

// layout-identical to ow_solid_hit / ow_solid_cast_options in include/ocean_waves.h
struct SolidHit {
    float t;
    float position[3];
    float normal[3];
    int32_t status;
    int32_t instance, triangle;
    float barycentric[2];
    uint32_t reserved[4];
};
struct SolidCastOptions {
    uint32_t flags;
    int32_t cull;
    uint32_t reserved[6];
};
static_assert(sizeof(SolidHit) == 64 && offsetof(SolidHit, status) == 28 && offsetof(SolidHit, barycentric) == 40 && sizeof(SolidCastOptions) == 32,
              "record layout");

constexpr uint32_t kSolidCastTwoSided = 1u;       // OW_SOLID_CAST_TWO_SIDED
constexpr uint64_t kSolidCastNoHit = ~(uint64_t)0;
constexpr float kSolidCastNoSlab = 3.4028235e38f;  // ray_setup's "the whole ray"

struct SolidCastParams {
    int two_sided;
    int cull;  // 1: the sphere test; 0: every instance that is not skipped goes on
};

// the shape, as the kernel and the CPU build read it
struct SolidCastShape {
    const float *local;      // [num_vertices][3]
    const int32_t *indices;  // [num_triangles][3]
    int num_vertices, num_triangles;
};

// an instance's sphere for one call: radius < 0 marks a skipped instance (a NaN or an Inf passes every test)
struct SolidCastBound {
    float c[3];
    float r;
};
static_assert(sizeof(SolidCastBound) == 16, "record layout");

// ---- the bounds ----

// One lane's share of the shape's box: the finite vertices lane, lane + 64, ... (a vertex that is not finite makes every triangle it is in
// non-finite in the world, whatever the transform: it bounds nothing).  lo > hi: the lane saw none.
OW_DEV void solid_cast_box_lane(const float *local, int num_vertices, int lane, float lo[3], float hi[3]) {
    for (int k = 0; k < 3; ++k) {
        lo[k] = 3.4028235e38f;
        hi[k] = -3.4028235e38f;
    }
    for (int v = lane; v < num_vertices; v += 64) {
        const float *l = local + 3 * (size_t)v;
        if (!(mesh_finite(l[0]) && mesh_finite(l[1]) && mesh_finite(l[2]))) continue;
        for (int k = 0; k < 3; ++k) {
            lo[k] = l[k] < lo[k] ? l[k] : lo[k];
            hi[k] = l[k] > hi[k] ? l[k] : hi[k];
        }
    }
}
// the middle of the box (halved first: no overflow); an empty box has its middle at 0
OW_DEV void solid_cast_box_centre(const float lo[3], const float hi[3], float c[3]) {
    for (int k = 0; k < 3; ++k) c[k] = lo[k] <= hi[k] ? 0.5f * lo[k] + 0.5f * hi[k] : 0.0f;
}
// one lane's share of the largest squared distance from c
OW_DEV float solid_cast_radius_lane(const float *local, int num_vertices, int lane, const float c[3]) {
    float m = 0.0f;
    for (int v = lane; v < num_vertices; v += 64) {
        const float *l = local + 3 * (size_t)v;
        if (!(mesh_finite(l[0]) && mesh_finite(l[1]) && mesh_finite(l[2]))) continue;
        const float x = l[0] - c[0], y = l[1] - c[1], z = l[2] - c[2];
        const float d2 = (x * x + y * y) + z * z;
        m = d2 > m ? d2 : m;
    }
    return m;
}
// The shape's sphere from the centre and the largest squared distance: the radius a little over the computed one (the distances carry a
// few ulp of relative error each).  An overflow gives an infinite radius, which passes every test.
OW_DEV SolidCastBound solid_cast_shape_sphere(const float c[3], float d2max) {
    SolidCastBound b;
    for (int k = 0; k < 3; ++k) b.c[k] = c[k];
    b.r = sqrtf(d2max) * 1.0001f;
    return b;
}

// An instance's sphere.  Every world vertex w = fl(B l + origin) lies within |B|_F |l - c| of B c + origin, and its FP32 evaluation (three
// products, three sums, each rounded) within 6 * 2^-24 (|B|_F |l| + |origin_k|) of that per component, as does the evaluated centre; |l| <=
// |c| + r.  kSolidCastRounding = 2^-18 covers both with a factor to spare, the floor covers products that underflow.
constexpr float kSolidCastRounding = 3.814697265625e-6f;
OW_DEV SolidCastBound solid_cast_instance_bound(const float *t, bool ok, const SolidCastBound &shape) {
    SolidCastBound b;
    b.c[0] = b.c[1] = b.c[2] = 0.0f;
    b.r = -1.0f;
    if (!ok) return b;
    solid_world(t, shape.c, b.c);
    float f2 = 0.0f;
    for (int k = 0; k < 9; ++k) f2 += t[k] * t[k];
    const float F = sqrtf(f2) * 1.0001f;
    const float lmax = sqrtf((shape.c[0] * shape.c[0] + shape.c[1] * shape.c[1]) + shape.c[2] * shape.c[2]) * 1.0001f + shape.r;
    const float omax = (fabsf(t[9]) + fabsf(t[10])) + fabsf(t[11]);
    b.r = (shape.r * F) * 1.0001f + (kSolidCastRounding * (F * lmax + omax) + 1e-30f);
    if (!(mesh_finite(b.c[0]) && mesh_finite(b.c[1]) && mesh_finite(b.c[2]))) b.r = 3.4028235e38f;  // no centre: everything passes
    return b;
}

// Can the ray meet anything inside the sphere at 0 <= t <= T?  In FP64.  The triangles the pairs see are those of p_k = fl(w_k - o): each
// within 2^-24 |w_k - o| per component of the world triangle, so the radius grows by 2^-21 (|C - o| + r) first; the FP64 rounding of the
// test itself is covered by 1e-14 of the squared distance.  Every comparison is false for a NaN: what cannot be decided passes.
OW_DEV bool solid_cast_sphere_pass(const SolidCastBound &b, const RaySetup &s, float T) {
    if (b.r < 0.0f) return false;  // skipped
    const double mx = (double)b.c[0] - (double)s.o[0], my = (double)b.c[1] - (double)s.o[1], mz = (double)b.c[2] - (double)s.o[2];
    const double dx = s.d[0], dy = s.d[1], dz = s.d[2];
    const double mm = (mx * mx + my * my) + mz * mz, dd = (dx * dx + dy * dy) + dz * dz, bb = (mx * dx + my * dy) + mz * dz;
    const double dist = sqrt(mm), sd = sqrt(dd);
    const double R = (double)b.r + 4.76837158203125e-7 * (dist + (double)b.r);
    const double slack = 1e-14 * mm;
    const bool off_line = mm - bb * bb / dd > R * R + slack;              // the line passes the sphere by
    const bool behind = bb + R * sd < -1e-7 * (dist * sd);               // every point of the sphere has t < 0
    const bool beyond = (bb - R * sd) / dd > (double)T * (1.0 + 1e-6);  // every point of the sphere has t > T
    return !(off_line || behind || beyond);
}

// ---- one pair ----

struct SolidCastPair {
    bool hit;
    float t;
    double e[3];  // e0, e1, e2
    double dn;
    float w[3][3];  // the world vertices
};

OW_DEV SolidCastPair solid_cast_pair(const SolidCastShape &shape, const float *transform, const RaySetup &s, float T, int two_sided, int triangle) {
    SolidCastPair r;
    r.hit = false;
    r.t = 0.0f;
    r.e[0] = r.e[1] = r.e[2] = r.dn = 0.0;
    const int32_t *idx = shape.indices + 3 * (size_t)triangle;
    bool ok = true;
    float p[3][3];
    for (int v = 0; v < 3; ++v) {
        ok = solid_world(transform, shape.local + 3 * (size_t)idx[v], r.w[v]) && ok;
        for (int k = 0; k < 3; ++k) p[v][k] = r.w[v][k] - s.o[k];
    }
    if (!ok) return r;
    const double p0x = p[0][0], p0y = p[0][1], p0z = p[0][2], p1x = p[1][0], p1y = p[1][1], p1z = p[1][2], p2x = p[2][0], p2y = p[2][1], p2z = p[2][2];
    const double dx = s.d[0], dy = s.d[1], dz = s.d[2];
    const double ax = p1x - p0x, ay = p1y - p0y, az = p1z - p0z, bx = p2x - p0x, by = p2y - p0y, bz = p2z - p0z;
    const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    r.e[0] = (dx * (p1y * p2z - p1z * p2y) + dy * (p1z * p2x - p1x * p2z)) + dz * (p1x * p2y - p1y * p2x);
    r.e[1] = (dx * (p2y * p0z - p2z * p0y) + dy * (p2z * p0x - p2x * p0z)) + dz * (p2x * p0y - p2y * p0x);
    r.e[2] = (dx * (p0y * p1z - p0z * p1y) + dy * (p0z * p1x - p0x * p1z)) + dz * (p0x * p1y - p0y * p1x);
    r.dn = (dx * nx + dy * ny) + dz * nz;
    bool inside;
    if (r.dn < 0.0) inside = r.e[0] <= 0.0 && r.e[1] <= 0.0 && r.e[2] <= 0.0;
    else if (r.dn > 0.0) inside = two_sided && r.e[0] >= 0.0 && r.e[1] >= 0.0 && r.e[2] >= 0.0;
    else inside = false;  // parallel, or a NaN
    if (!inside) return r;
    float t = (float)(((p0x * nx + p0y * ny) + p0z * nz) / r.dn);
    if (t == 0.0f) t = 0.0f;  // -0 -> +0
    if (!(t >= 0.0f && t <= T)) return r;
    r.hit = true;
    r.t = t;
    return r;
}

OW_DEV uint64_t solid_cast_word(float t, int pair) {
    uint32_t bits;
    __builtin_memcpy(&bits, &t, 4);
    return ((uint64_t)bits << 32) | (uint32_t)pair;
}

// the index of the j-th set bit of m (j < the number of set bits)
OW_DEV int solid_cast_select(uint64_t m, int j) {
    int pos = 0;
    for (int w = 32; w >= 1; w >>= 1) {
        const int c = bit_count(m & ((((uint64_t)1 << w) - 1) << pos));
        if (j >= c) {
            j -= c;
            pos += w;
        }
    }
    return pos;
}

OW_DEV SolidHit solid_hit_zero() {
    SolidHit h;
    __builtin_memset(&h, 0, sizeof(h));
    return h;
}

// the limit of one ray: max_distance, or the water's t where its record (of which the cast reads these two words) has a hit that is nearer
OW_DEV float solid_cast_limit(const Ray &ray, bool has_water, float water_t, int32_t water_status) {
    float T = ray.max_distance;
    if (has_water && (water_status & kRayHit) && water_t < T) T = water_t;
    return T;
}

// the winner's record, rebuilt from its word
OW_DEV SolidHit solid_cast_record(const SolidCastShape &shape, const SolidInstances &in, const RaySetup &s, float T, int two_sided, uint64_t word) {
    SolidHit h = solid_hit_zero();
    h.instance = h.triangle = -1;
    if (word == kSolidCastNoHit) return h;
    const SolidSplit at = solid_split((int)(uint32_t)word, shape.num_triangles);
    const SolidCastPair pr = solid_cast_pair(shape, solid_transform(in, at.instance), s, T, two_sided, at.item);
    h.t = pr.t;
    for (int k = 0; k < 3; ++k) {
        const float x = s.o[k] + pr.t * s.d[k];
        h.position[k] = x > 3.4028235e38f ? 3.4028235e38f : (x < -3.4028235e38f ? -3.4028235e38f : x);
    }
    float n[3];
    solid_normal(pr.w[0], pr.w[1], pr.w[2], pr.dn > 0.0 ? -1.0 : 1.0, n);
    const bool n_ok = mesh_finite(n[0]) && mesh_finite(n[1]) && mesh_finite(n[2]);
    for (int k = 0; k < 3; ++k) h.normal[k] = n_ok ? n[k] : 0.0f;
    h.status = kRayHit | kRaySolid;
    h.instance = at.instance;
    h.triangle = at.item;
    const double se = (pr.e[0] + pr.e[1]) + pr.e[2];
    if (se != 0.0) {
        const float b1 = (float)(pr.e[1] / se), b2 = (float)(pr.e[2] / se);
        h.barycentric[0] = mesh_finite(b1) ? b1 : 0.0f;
        h.barycentric[1] = mesh_finite(b2) ? b2 : 0.0f;
    }
    return h;
}

// ---- one ray ----
// Wave is the 64 lanes: wave.ballot(pred) is the mask of the lanes j where pred(j) holds; wave.lanes(fn) has every lane j run fn(j, best_j),
// best_j being the lane's smallest word so far; wave.min_best() is the smallest of them.  Everything here outside pred and fn is
// wave-uniform.  passed, pairs: the instances that went on to their triangles, and the pairs tested (the counters of ow_cast_stats).
struct SolidCastWinner {
    RaySetup s;
    float T;
    uint64_t word;  // kSolidCastNoHit: none
};
template <class Wave>
OW_DEV SolidCastWinner solid_cast_search(Wave &wave, const SolidCastShape &shape, const SolidInstances &in, const SolidCastBound *bounds,
                                         const SolidCastParams &cp, const Ray &ray, bool has_water, float water_t, int32_t water_status, uint64_t &passed,
                                         uint64_t &pairs) {
    passed = pairs = 0;
    SolidCastWinner win;
    win.s = ray_setup(ray, kSolidCastNoSlab, 0.0f);
    win.T = 0.0f;
    win.word = kSolidCastNoHit;
    if (!win.s.valid) return win;
    const RaySetup &s = win.s;
    const float T = win.T = solid_cast_limit(ray, has_water, water_t, water_status);
    const int nt = shape.num_triangles;
    for (int base = 0; base < in.count; base += 64) {
        const uint64_t m = wave.ballot([&](int j) {
            const int i = base + j;
            if (i >= in.count) return false;
            const SolidCastBound b = bounds[i];
            return cp.cull ? solid_cast_sphere_pass(b, s, T) : !(b.r < 0.0f);
        });
        if (!m) continue;
        const int n = bit_count(m), work = n * nt;  // <= 64 * 65536
        passed += (uint64_t)n;
        pairs += (uint64_t)work;
        wave.lanes([&](int j, uint64_t &best) {
            for (int f = j; f < work; f += 64) {
                const int k = f / nt, tri = f - k * nt;
                const int inst = base + solid_cast_select(m, k);
                const SolidCastPair pr = solid_cast_pair(shape, solid_transform(in, inst), s, T, cp.two_sided, tri);
                if (!pr.hit) continue;
                const uint64_t word = solid_cast_word(pr.t, inst * nt + tri);
                best = word < best ? word : best;
            }
        });
    }
    win.word = wave.min_best();
    return win;
}
// the ray's record from the search's result (one lane's work)
OW_DEV SolidHit solid_cast_finish(const SolidCastShape &shape, const SolidInstances &in, const SolidCastParams &cp, const SolidCastWinner &win) {
    if (!win.s.valid) {
        SolidHit h = solid_hit_zero();
        h.status = kRayInvalid;
        return h;
    }
    return solid_cast_record(shape, in, win.s, win.T, cp.two_sided, win.word);
}

// The 64 lanes stepped one after the other (the CPU build).
struct SolidCastSerialWave {
    uint64_t best[64];
    SolidCastSerialWave() {
        for (int j = 0; j < 64; ++j) best[j] = kSolidCastNoHit;
    }
    template <class Pred>
    uint64_t ballot(const Pred &pred) {
        uint64_t m = 0;
        for (int j = 0; j < 64; ++j)
            if (pred(j)) m |= (uint64_t)1 << j;
        return m;
    }
    template <class Fn>
    void lanes(const Fn &fn) {
        for (int j = 0; j < 64; ++j) fn(j, best[j]);
    }
    uint64_t min_best() const {
        uint64_t m = kSolidCastNoHit;
        for (int j = 0; j < 64; ++j) m = best[j] < m ? best[j] : m;
        return m;
    }
};

}  // namespace ow

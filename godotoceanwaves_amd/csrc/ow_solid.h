// ow_solid.h -- opaque triangle meshes drawn at instance transforms into a camera view (include/ocean_waves.h ow_solid_*): the floating
// bodies of ow_bodies_* (or a caller's transforms) over a picture of ow_mesh_draw or ow_render_view, depth-tested against it and writing
// depth into it, so that the spray drawn afterwards (ow_spray_draw.h) is hidden behind them.
//
// Compiles as device code (ow_solid.hip, built with -ffp-contract=off) and as plain C++ (tests/solid/, g++ -ffp-contract=off), like
// ow_mesh.h: every operation is an IEEE-754 add, subtract, multiply, divide, square root, min / max or compare, in FP32 or (the plane
// vectors and the shading normal) FP64, so both builds produce the same bits.
//
// Nothing of the coverage rule is restated here: the vertex records are MeshVertex records, and the set-up, the planes, the coverage test
// and the visibility word are ow_mesh.h's tri_setup, tri_planes, tri_cover and mesh_word, called as they are.
//
//   vertex    instance transform T (twelve floats, BuoyancyBody::transform's layout: basis rows [0..8], origin [9..11]), local vertex l:
//             w_k = ((T[3k] l_0 + T[3k+1] l_1) + T[3k+2] l_2) + T[9+k]   (solid_world: lever_arm's row product, then the origin)
//             V   = B^T (w - camera.position), mesh_vertex's operations in their order
//             A vertex whose w or V is not finite carries kMeshVertexNotFinite: its triangles are culled.  Every vertex of an instance
//             that is skipped (a transform value that is not finite, a body whose fault flag is raised) carries kSolidVertexSkipped as
//             well: its triangles are not counted as culled, the instance is counted once.
//   pair      (instance, triangle) pairs are numbered instance * num_triangles + triangle; that number is the low half of the visibility
//             word, so of all pairs that cover a pixel the smallest (depth bits, pair) wins whatever the order they are rastered in.
//   facing    det < 0 is the outward side (ow_mesh.h).  Back faces are culled by tri_setup (cull_back) unless the draw is two-sided; then
//             they are drawn with the normal negated.
//   planes    A triangle whose plane vectors are not all finite (view positions near the top of the FP32 range) is culled.
//   resolve   The winner's barycentrics are tri_cover's e_i / (e_0 + e_1 + e_2) (mesh_pixel's form); its distance along the pixel's
//             normalised ray is d = s sqrtf((x x + y y) + 1), ow_spray_draw.h's expression.  It is drawn when the record under it has no
//             kRayHit or d <= the record's t.  The water is opaque in this composite: what lies under it is hidden.
//   shading   n = (w1 - w0) x (w2 - w0) / |.|: the edges in FP32, the cross product, the length and the division in FP64, narrowed once
//             (negated for a back face); diffuse = light_color max(n . l^, 0) with dot3's order, l^ normalised by the host as
//             ow_shading.h's light is; color = albedo (diffuse + ambient_color).  No specular, no textures.
#pragma once

#include <cmath>

#include "ow_buoyancy.h"
#include "ow_mesh.h"

namespace ow {

// layout-identical to ow_solid_options in include/ocean_waves.h
struct SolidOptions {
    float near;
    float color[3];
    float light_direction[3];
    uint32_t flags;
    float light_color[3];
    float ambient_color[3];
    float background_color[3];
    int32_t lane_box;
    uint32_t reserved[14];
};
static_assert(sizeof(SolidOptions) == 128 && offsetof(SolidOptions, flags) == 28 && offsetof(SolidOptions, lane_box) == 68, "record layout");

constexpr int32_t kRaySolid = 16;                  // OW_RAY_SOLID
constexpr uint32_t kSolidTwoSided = 1u;            // OW_SOLID_TWO_SIDED
constexpr int kSolidMaxInstances = 65536;          // OW_SOLID_MAX_INSTANCES
constexpr int kSolidMaxTriangles = 65536;          // OW_SOLID_MAX_TRIANGLES
constexpr int64_t kSolidMaxProduct = 1 << 24;      // instances * triangles and instances * vertices per draw
constexpr uint32_t kSolidVertexSkipped = 2u;       // MeshVertex::flags: the vertex belongs to a skipped instance
constexpr float kSolidColorMax = 1.0e12f;          // the largest magnitude of a colour the options take: color stays finite
constexpr int kSolidTransformFloats = 12;

// what the four counters of a draw hold: skipped instances, then every triangle of the other instances as exactly one of three (in the
// order of ow_mesh.h's classes, which the host reads all such counters by)
enum : int { kSolidSkippedInstances = kTriSkipped, kSolidCulled = kTriCulled, kSolidLane = kTriLane, kSolidWave = kTriWave };

// a draw's constants, resolved once from the options
struct SolidParams {
    MeshParams mp;          // near, cull_back (not two-sided), lane_box, camera_ok; the query settings are not read
    float albedo[3];
    float light[3];         // the unit vector towards the light (normalised in FP64 on the host)
    float light_color[3], ambient_color[3], background[3];
    int two_sided;
};

// where the instances of a draw come from: transforms `stride` floats apart (a body set's pose records, or an uploaded array) and, for a
// body set, the fault flags beside them
struct SolidInstances {
    const float *transforms;  // instance i's twelve floats start at transforms + i * stride
    const int32_t *flags;     // [count] or nullptr: != 0 skips the instance
    int stride;               // in floats
    int count;
};

// ---- the instance front end: what the draw and the shadow cast (ow_shadow.h), on the device and in the CPU builds of both, do ahead of
// their own arithmetic -- which (instance, vertex) or (instance, triangle) a flat index is, where that instance's transform lies, whether
// the instance is drawn at all, and where it puts a local vertex in the world ----

// flat index -> (instance, item) with `per_instance` vertices or triangles each: flat = instance * per_instance + item
struct SolidSplit {
    int instance, item;
};
OW_DEV SolidSplit solid_split(int flat, int per_instance) {
    const int instance = flat / per_instance;
    return SolidSplit{instance, flat - instance * per_instance};
}

OW_DEV const float *solid_transform(const SolidInstances &in, int instance) { return in.transforms + (size_t)instance * in.stride; }

// drawn: every float of the transform is finite and, for a body, its fault flag is down
OW_DEV bool solid_instance_ok(const float *t, const int32_t *flag) {
    bool ok = !flag || *flag == 0;
    for (int k = 0; k < kSolidTransformFloats; ++k) ok = ok && mesh_finite(t[k]);
    return ok;
}
OW_DEV bool solid_instance_ok(const SolidInstances &in, int instance) {
    return solid_instance_ok(solid_transform(in, instance), in.flags ? in.flags + instance : nullptr);
}

// the world position of local vertex l under transform t, and whether it is finite: lever_arm's row product, then the origin.  The draw
// and the cast both take it from here, so a caster's vertex is where the drawn one is to the bit.
OW_DEV bool solid_world(const float *t, const float l[3], float w[3]) {
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        w[k] = ((t[3 * k] * l[0] + t[3 * k + 1] * l[1]) + t[3 * k + 2] * l[2]) + t[9 + k];
        ok = ok && mesh_finite(w[k]);
    }
    return ok;
}

// the three vertex records of pair `pair` (MeshVertex for the draw, ShadowVertex for the cast)
template <typename Vertex>
struct SolidTriangle {
    const Vertex *a, *b, *c;
};
template <typename Vertex>
OW_DEV SolidTriangle<Vertex> solid_triangle(const int32_t *indices, int num_vertices, int num_triangles, const Vertex *verts, int pair) {
    const SolidSplit at = solid_split(pair, num_triangles);
    const Vertex *base = verts + (size_t)at.instance * num_vertices;
    return SolidTriangle<Vertex>{base + indices[3 * (size_t)at.item], base + indices[3 * (size_t)at.item + 1], base + indices[3 * (size_t)at.item + 2]};
}

// one (instance, vertex): the record tri_setup reads
OW_DEV MeshVertex solid_vertex(const float *t, bool instance_ok, const float l[3], const CameraParams &cam, const MeshParams &mp) {
    MeshVertex out;
    out.wave_height = out.uv[0] = out.uv[1] = out.falloff = 0.0f;
    out.reserved = 0u;
    for (int k = 0; k < 3; ++k) out.position[k] = out.view[k] = 0.0f;
    if (!instance_ok) {
        out.flags = kMeshVertexNotFinite | kSolidVertexSkipped;
        return out;
    }
    bool ok = solid_world(t, l, out.position);
    float rel[3];
    for (int k = 0; k < 3; ++k) rel[k] = out.position[k] - cam.o[k];
    if (mp.camera_ok)
        for (int k = 0; k < 3; ++k) {
            out.view[k] = (cam.B[k] * rel[0] + cam.B[3 + k] * rel[1]) + cam.B[6 + k] * rel[2];  // column k of B
            ok = ok && mesh_finite(out.view[k]);
        }
    out.flags = ok ? 0u : kMeshVertexNotFinite;
    if (!ok)  // the record itself stays finite: the flag says what happened
        for (int k = 0; k < 3; ++k) out.position[k] = out.view[k] = 0.0f;
    return out;
}

OW_DEV bool solid_planes_finite(const TriPlanes &p) {
    bool ok = mesh_finite(p.det);
    for (int a = 0; a < 3; ++a) {
        ok = ok && mesh_finite(p.N[a]);
        for (int b = 0; b < 3; ++b) ok = ok && mesh_finite(p.n[a][b]);
    }
    return ok;
}

// tri_setup for one pair, and the counter it falls under: kSolidCulled, kSolidLane, kSolidWave, or -1 for a triangle of a skipped instance.
// s.kind is kTriLane or kTriWave exactly where the counter is kSolidLane or kSolidWave.
OW_DEV TriSetup solid_setup(const SolidTriangle<MeshVertex> &t, const CameraParams &cam, const MeshParams &mp, int &counter) {
    TriSetup s = tri_setup(*t.a, *t.b, *t.c, cam, mp);
    if ((s.kind == kTriLane || s.kind == kTriWave) && !solid_planes_finite(s.p)) s.kind = kTriCulled;
    counter = s.kind == kTriLane ? kSolidLane : (s.kind == kTriWave ? kSolidWave : kSolidCulled);
    if (s.kind == kTriSkipped && ((t.a->flags | t.b->flags | t.c->flags) & kSolidVertexSkipped)) counter = -1;
    return s;
}

// The unit normal of the world triangle (a, b, c), times sg (-1: a back face, the side that is seen): the edges in FP32, the cross product,
// the length and the division in FP64, narrowed once; zeros for a triangle without area.  The draw's shading normal and the ray cast's
// (ow_solid_cast.h) are both this.
OW_DEV void solid_normal(const float a[3], const float b[3], const float c[3], double sg, float n[3]) {
    float e1[3], e2[3];
    for (int k = 0; k < 3; ++k) {
        e1[k] = b[k] - a[k];
        e2[k] = c[k] - a[k];
    }
    const double ax = e1[0], ay = e1[1], az = e1[2], bx = e2[0], by = e2[1], bz = e2[2];
    const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    n[0] = n[1] = n[2] = 0.0f;
    if (len > 0.0) {
        n[0] = (float)(sg * nx / len);
        n[1] = (float)(sg * ny / len);
        n[2] = (float)(sg * nz / len);
    }
}

// One pixel from its visibility word against the record under it (bg_t, bg_status; 0, 0 without records).  drawn: a solid is drawn, and
// what is returned is the pixel's whole record.  Otherwise the pixel keeps what it had (and zeros are returned).
OW_DEV RenderPixel solid_pixel(const SolidParams &sp, const CameraParams &cam, uint64_t word, const int32_t *indices, int num_vertices, int num_triangles,
                               const MeshVertex *verts, int i, int j, float bg_t, int32_t bg_status, bool &drawn) {
    RenderPixel px = render_pixel_zero();
    drawn = false;
    if (!sp.mp.camera_ok || word == kMeshNoTriangle) return px;
    const int pair = (int)(uint32_t)word;
    const SolidTriangle<MeshVertex> tr = solid_triangle(indices, num_vertices, num_triangles, verts, pair);
    const MeshVertex a = *tr.a, b = *tr.b, c = *tr.c;
    const TriPlanes p = tri_planes(a.view, b.view, c.view);
    const TriCover cv = tri_cover(p, cam, sp.mp.near, i, j);
    float x, y;
    mesh_pixel_xy(cam, i, j, x, y);
    const float d = cv.depth * sqrtf((x * x + y * y) + 1.0f);
    if (!mesh_finite(d)) return px;
    if ((bg_status & kRayHit) && !(d <= bg_t)) return px;
    const float se = (cv.e[0] + cv.e[1]) + cv.e[2];
    float w0 = 1.0f, w1 = 0.0f, w2 = 0.0f;
    if (se != 0.0f) {
        w0 = cv.e[0] / se;
        w1 = cv.e[1] / se;
        w2 = cv.e[2] / se;
    }
    px.t = d;
    px.status = kRayHit | kRaySolid;
    for (int k = 0; k < 3; ++k) px.position[k] = (w0 * a.position[k] + w1 * b.position[k]) + w2 * c.position[k];
    float n[3];
    solid_normal(a.position, b.position, c.position, p.det > 0.0f ? -1.0 : 1.0, n);  // a back face (two-sided draws only): the side that is seen
    const float ndl = fmaxf(dot3(n, sp.light), 0.0f);
    for (int k = 0; k < 3; ++k) {
        px.normal[k] = n[k];
        px.albedo[k] = sp.albedo[k];
        px.diffuse[k] = sp.light_color[k] * ndl;
        px.color[k] = sp.albedo[k] * (px.diffuse[k] + sp.ambient_color[k]);
    }
    const SolidSplit at = solid_split(pair, num_triangles);
    px.reserved[0] = (uint32_t)at.item + 1u;
    px.reserved[3] = (uint32_t)at.instance + 1u;
    drawn = true;
    return px;
}

}  // namespace ow

// ow_mesh.h -- a displaced water mesh drawn for a camera (include/ocean_waves.h ow_mesh_*): water.gdshader's vertex() (lines 27-39) over
// a caller's mesh, a visibility-buffer rasteriser, and the fragment() / light() of ow_shading.h on the varyings the rasteriser of the
// reference's engine would interpolate.  What the reference draws (water.gd:8-9,46: a clipmap mesh, linear between its vertices), where
// ow_render.h draws the limit surface.
//
// Compiles as device code (ow_mesh.hip, built with -ffp-contract=off) and as plain C++ (tests/mesh/, g++ -ffp-contract=off), like
// ow_render.h: every operation is an IEEE-754 add, subtract, multiply, divide, square root, floor / ceil, min / max or compare, in FP32
// or (a triangle's plane vectors) FP64, so both builds produce the same bits.
//
// Vertex stage.  w = local + origin, UV = w.xz, D = sample_point's displacement sum at UV (the same operations in the same order: the
// bits of ow_surface_sample.displacement), f = falloff_at around the options' centre, position = w + D f, wave_height = D.y before the
// factor (:38).  The view-space position is V = B^T (position - camera) (x right, y up, z back: the view depth is -V.z).
//
// Coverage.  The camera is the origin of view space and pixel (i, j)'s ray is r = (x, y, -1) with pixel_ray's own x and y.  For a triangle
// V0 V1 V2 the point where the ray meets its plane is s r = b0 V0 + b1 V1 + b2 V2 with
//     e_i = r . n_i,   n_0 = V1 x V2, n_1 = V2 x V0, n_2 = V0 x V1        (homogeneous edge functions: Olano & Greer 1997)
//     b_i = e_i / (e_0 + e_1 + e_2),   s = det / (r . N),   N = (V1 - V0) x (V2 - V0),   det = V0 . N
// and s is the view depth (r's z is -1).  The pixel is covered when every e_i has det's sign or is zero (edges are inclusive), r . N has
// det's sign, and near < s <= max_distance.  Nothing is projected, so a triangle that crosses the near plane or reaches behind the camera
// needs no clipping: the part of it with s <= near is never covered.  The b_i are barycentrics in space: interpolating with them is the
// perspective-correct interpolation.  The n_i, N and det are formed in FP64 from the FP32 view positions and rounded once: a cross
// product's rounding is then relative to the product itself, not to |V|^2.  a x b = -(b x a) holds to the bit, so the two triangles on a
// shared edge see edge functions that are each other's negation: a pixel centre is inside one of them or, exactly on the edge, both --
// never neither.  Of all triangles that cover a pixel the smallest (depth bits, triangle index) is drawn: a min over 64-bit words, the
// same whatever order the triangles come in.
//
// Facing.  The upper side of a triangle is the one N points to (counter-clockwise seen from there: the OBJ convention, the upper side of
// the reference's clipmap_low.obj): det < 0.  det > 0 is seen from the underside and carries kRayFromBelow; det == 0 (edge-on, or of
// zero area) covers nothing.
#pragma once

#include "ow_render.h"

namespace ow {

// layout-identical to ow_mesh_vertex in include/ocean_waves.h
struct MeshVertex {
    float position[3];
    float wave_height;
    float uv[2];
    float falloff;
    uint32_t reserved;
    float view[3];
    uint32_t flags;
};
static_assert(sizeof(MeshVertex) == 48 && offsetof(MeshVertex, uv) == 16 && offsetof(MeshVertex, view) == 32, "record layout");

constexpr uint32_t kMeshVertexNotFinite = 1u;  // OW_MESH_VERTEX_NOT_FINITE
constexpr float kMeshDefaultNear = 0.05f;      // Camera3D.near
constexpr int kMeshLaneBox = 4;                // a pixel box of at most this many centres a side is walked by the triangle's own lane
constexpr uint64_t kMeshNoTriangle = ~(uint64_t)0;
constexpr float kMeshDepthSlack = 0.000244140625f;  // 2^-12: how far tri_setup's box reaches past near and max_distance, relative to either

struct MeshParams {
    QueryParams qp;    // the falloff flag and centre; the solver's settings are not read
    float near;        // > 0
    int cull_back;     // OW_MESH_CULL_BACK
    int lane_box;      // kMeshLaneBox, or what a measurement asks for (0: every triangle goes to the wave)
    int camera_ok;     // 0: the camera is not finite -- nothing is drawn and every pixel carries kRayInvalid
};
// the lane_box of an options record (-1 .. 64, checked by the host) as a set-up reads it: 0 selects the default, -1 sends every triangle to the wave
inline int mesh_lane_box(int32_t option) { return option == 0 ? kMeshLaneBox : (option < 0 ? 0 : option); }

// what the four counters of a draw add up over: every triangle is exactly one of these
enum : int { kTriSkipped = 0, kTriCulled = 1, kTriLane = 2, kTriWave = 3 };

OW_HD bool mesh_finite(float v) { return fabsf(v) <= 3.4028235e38f; }  // false for a NaN

// the camera as the draw needs it: finite, a positive far distance and field of view
OW_HD bool mesh_camera_ok(const CameraParams &cam) {
    bool ok = mesh_finite(cam.tan_half_fov) && mesh_finite(cam.aspect) && mesh_finite(cam.max_distance) && cam.max_distance > 0.0f &&
              cam.tan_half_fov > 0.0f && cam.aspect > 0.0f;
    for (int k = 0; k < 3; ++k) ok = ok && mesh_finite(cam.o[k]);
    for (int k = 0; k < 9; ++k) ok = ok && mesh_finite(cam.B[k]);
    return ok;
}

// water.gdshader:27-39 for one vertex, and its view-space position (zeros without a camera, or with one that is not finite)
OW_DEV MeshVertex mesh_vertex(const u16x4 *disp, int n, int cascades, const SurfaceScales &scales, const MeshParams &mp, const CameraParams &cam,
                              bool has_camera, const float local[3], const float origin[3]) {
    MeshVertex out;
    float w[3];
    for (int k = 0; k < 3; ++k) w[k] = local[k] + origin[k];
    float dsum[3] = {0.0f, 0.0f, 0.0f};
    const size_t plane = (size_t)n * n;
    for (int c = 0; c < cascades; ++c) {  // sample_point's displacement sum, operation for operation
        const float sx = scales.s[c][0], sy = scales.s[c][1], sz = scales.s[c][2];
        const Tap t = make_tap(clamp_coord(w[0] * sx), clamp_coord(w[2] * sy), n);
        float d[4];
        bilinear(disp + c * plane, n, t, d);
        for (int k = 0; k < 3; ++k) dsum[k] += d[k] * sz;
    }
    float grad[2];
    const float f = falloff_at(mp.qp, w[0], w[2], grad);
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        out.position[k] = w[k] + dsum[k] * f;
        ok = ok && mesh_finite(out.position[k]);
    }
    out.wave_height = dsum[1];
    ok = ok && mesh_finite(dsum[1]);
    out.uv[0] = w[0];
    out.uv[1] = w[2];
    out.falloff = f;
    out.reserved = 0u;
    out.view[0] = out.view[1] = out.view[2] = 0.0f;
    if (has_camera && mp.camera_ok) {
        float rel[3];
        for (int k = 0; k < 3; ++k) rel[k] = out.position[k] - cam.o[k];
        for (int k = 0; k < 3; ++k) {
            out.view[k] = (cam.B[k] * rel[0] + cam.B[3 + k] * rel[1]) + cam.B[6 + k] * rel[2];   // column k of B
            ok = ok && mesh_finite(out.view[k]);
        }
    }
    out.flags = ok ? 0u : kMeshVertexNotFinite;
    if (!ok) {  // the record itself stays finite: the flag says what happened
        for (int k = 0; k < 3; ++k) out.position[k] = out.view[k] = 0.0f;
        out.uv[0] = out.uv[1] = out.wave_height = 0.0f;
        out.falloff = 1.0f;
    }
    return out;
}

// pixel_ray's x and y: the ray of pixel (i, j) is (x, y, -1) in view space
OW_DEV void mesh_pixel_xy(const CameraParams &cam, int i, int j, float &x, float &y) {
    x = ((2.0f * ((float)i + 0.5f)) / (float)cam.width - 1.0f) * cam.aspect * cam.tan_half_fov;
    y = (1.0f - (2.0f * ((float)j + 0.5f)) / (float)cam.height) * cam.tan_half_fov;
}

// a triangle's plane vectors: what coverage, depth and the barycentrics are computed from, in the raster kernel and in the shade kernel
struct TriPlanes {
    float n[3][3];  // n_i
    float N[3];
    float det;
};
OW_DEV void mesh_cross64(const float a[3], const float b[3], float out[3]) {
    const double ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2];
    out[0] = (float)(ay * bz - az * by);
    out[1] = (float)(az * bx - ax * bz);
    out[2] = (float)(ax * by - ay * bx);
}
OW_DEV TriPlanes tri_planes(const float V0[3], const float V1[3], const float V2[3]) {
    TriPlanes p;
    mesh_cross64(V1, V2, p.n[0]);
    mesh_cross64(V2, V0, p.n[1]);
    mesh_cross64(V0, V1, p.n[2]);
    const double ax = (double)V1[0] - V0[0], ay = (double)V1[1] - V0[1], az = (double)V1[2] - V0[2];
    const double bx = (double)V2[0] - V0[0], by = (double)V2[1] - V0[1], bz = (double)V2[2] - V0[2];
    const double Nx = ay * bz - az * by, Ny = az * bx - ax * bz, Nz = ax * by - ay * bx;
    p.N[0] = (float)Nx;
    p.N[1] = (float)Ny;
    p.N[2] = (float)Nz;
    p.det = (float)((V0[0] * Nx + V0[1] * Ny) + V0[2] * Nz);
    return p;
}

// one pixel centre against one triangle
struct TriCover {
    bool hit;
    float e[3];
    float depth;
};
OW_DEV TriCover tri_cover(const TriPlanes &p, const CameraParams &cam, float near, int i, int j) {
    float x, y;
    mesh_pixel_xy(cam, i, j, x, y);
    TriCover c;
    for (int k = 0; k < 3; ++k) c.e[k] = (x * p.n[k][0] + y * p.n[k][1]) - p.n[k][2];
    const float rn = (x * p.N[0] + y * p.N[1]) - p.N[2];
    const float sg = p.det < 0.0f ? -1.0f : 1.0f;
    c.depth = p.det / rn;
    c.hit = sg * c.e[0] >= 0.0f && sg * c.e[1] >= 0.0f && sg * c.e[2] >= 0.0f && sg * rn > 0.0f && c.depth > near && c.depth <= cam.max_distance;
    return c;
}
OW_DEV uint64_t mesh_word(float depth, int tri) {
    uint32_t bits;
    __builtin_memcpy(&bits, &depth, 4);
    return ((uint64_t)bits << 32) | (uint32_t)tri;
}

// A triangle's set-up: its class and, for the two drawn classes, the planes and the box of pixel centres that may be covered.  The box
// is that of the triangle's part in front of the near plane (its corners and the points where its edges cross z = -near), projected and
// widened by what the projection's rounding can move a corner -- a sixteenth of a pixel, and for a triangle that crosses the near plane the
// error of the crossing points magnified by 1 / near -- then clamped to the image.  A box that holds no pixel centre is culled.  The plane
// the box is cut at lies kMeshDepthSlack inside the near plane, and a triangle counts as beyond the far distance only that much past it:
// with the planes themselves a triangle whose depths lie within a few ulp of near (or of max_distance) had centres covered outside its
// box, or was culled whole, because the depth tri_cover tests is itself rounded (tests/test_raster_edges.py, the `near` and `far` families; profiles/raster_edges.txt).
struct TriSetup {
    TriPlanes p;
    int x0, x1, y0, y1;
    int kind;
};
OW_DEV int mesh_box_edge(float v, float lo, float hi, bool up) {  // v clamped in float first: the conversion's operand is always in range
    const float c = fminf(fmaxf(v, lo), hi);                      // a NaN reads as lo
    return (int)(up ? ceilf(c) : floorf(c));
}
OW_DEV TriSetup tri_setup(const MeshVertex &a, const MeshVertex &b, const MeshVertex &c, const CameraParams &cam, const MeshParams &mp) {
    TriSetup s;
    s.x0 = s.y0 = 0;
    s.x1 = s.y1 = -1;
    s.kind = kTriSkipped;
    __builtin_memset(&s.p, 0, sizeof(s.p));
    if ((a.flags | b.flags | c.flags) & kMeshVertexNotFinite) return s;
    s.kind = kTriCulled;
    if (!mp.camera_ok) return s;
    s.p = tri_planes(a.view, b.view, c.view);
    if (!(s.p.det != 0.0f) || (mp.cull_back && s.p.det > 0.0f)) return s;
    const float *V[3] = {a.view, b.view, c.view};
    // tri_cover compares a rounded depth (det / rn in FP32) with near and max_distance, so a centre whose exact depth is a few ulp on the
    // wrong side of either can still be covered: the box is cut at planes kMeshDepthSlack inside near and beyond max_distance
    const float zc = mp.near * (1.0f - kMeshDepthSlack), zfar = cam.max_distance * (1.0f + kMeshDepthSlack);
    const float sxp = (float)cam.width / (2.0f * cam.aspect * cam.tan_half_fov), syp = (float)cam.height / (2.0f * cam.tan_half_fov);
    const float hx = 0.5f * (float)cam.width, hy = 0.5f * (float)cam.height;
    float lox = 3.0e38f, hix = -3.0e38f, loy = 3.0e38f, hiy = -3.0e38f, vmax = 0.0f;
    bool any = false, straddle = false, all_far = true;
    for (int k = 0; k < 3; ++k) {
        const float z = -V[k][2];
        vmax = fmaxf(vmax, fmaxf(fabsf(V[k][0]), fmaxf(fabsf(V[k][1]), fabsf(z))));
        all_far = all_far && z > zfar;
        if (z > zc) {
            const float cx = (V[k][0] / z) * sxp + hx, cy = hy - (V[k][1] / z) * syp;
            lox = fminf(lox, cx);
            hix = fmaxf(hix, cx);
            loy = fminf(loy, cy);
            hiy = fmaxf(hiy, cy);
            any = true;
        }
        const float *P = V[k], *Q = V[(k + 1) % 3];
        const float zp = -P[2], zq = -Q[2];
        if ((zp > zc) != (zq > zc)) {
            const float t = (zc - zp) / (zq - zp);
            const float px = P[0] + t * (Q[0] - P[0]), py = P[1] + t * (Q[1] - P[1]);
            const float cx = (px / zc) * sxp + hx, cy = hy - (py / zc) * syp;
            lox = fminf(lox, cx);
            hix = fmaxf(hix, cx);
            loy = fminf(loy, cy);
            hiy = fmaxf(hiy, cy);
            straddle = true;
        }
    }
    if (!any || all_far) return s;  // wholly behind the near plane, or wholly beyond the far distance
    const float pad = 0.0625f + (straddle ? 1.0f + (vmax * 4.0e-7f / zc) * fmaxf(sxp, syp) : 0.0f);
    const float W = (float)cam.width, H = (float)cam.height;
    s.x0 = mesh_box_edge(lox - 0.5f - pad, 0.0f, W, true);
    s.x1 = mesh_box_edge(hix - 0.5f + pad, -1.0f, W - 1.0f, false);
    s.y0 = mesh_box_edge(loy - 0.5f - pad, 0.0f, H, true);
    s.y1 = mesh_box_edge(hiy - 0.5f + pad, -1.0f, H - 1.0f, false);
    if (s.x0 > s.x1 || s.y0 > s.y1) return s;
    s.kind = (s.x1 - s.x0 < mp.lane_box && s.y1 - s.y0 < mp.lane_box) ? kTriLane : kTriWave;
    return s;
}

// One pixel of the picture from its visibility word: the record and the RGBA8 word.  `t` is the distance along the pixel's normalised ray,
// `p` the interpolated UV, reserved[0] the triangle's index + 1 (0: none).
OW_DEV RenderPixel mesh_pixel(const u16x4 *disp, const u16x4 *norm, int n, int cascades, const SurfaceScales &scales, const CameraParams &cam,
                              const ShadeParams &sp, const MeshParams &mp, uint64_t word, const int32_t *indices, const MeshVertex *verts, int i,
                              int j, uint32_t *rgba) {
    RenderPixel px = render_pixel_zero();
    if (!mp.camera_ok || word == kMeshNoTriangle) {
        px.status = mp.camera_ok ? 0 : kRayInvalid;
        for (int k = 0; k < 3; ++k) px.color[k] = sp.sky_color[k];
        *rgba = pack_rgba8(px.color);
        return px;
    }
    const int tri = (int)(uint32_t)word;
    const MeshVertex a = verts[indices[3 * (size_t)tri]], b = verts[indices[3 * (size_t)tri + 1]], c = verts[indices[3 * (size_t)tri + 2]];
    const TriPlanes p = tri_planes(a.view, b.view, c.view);
    const TriCover cv = tri_cover(p, cam, mp.near, i, j);
    const float se = (cv.e[0] + cv.e[1]) + cv.e[2];
    float w0 = 1.0f, w1 = 0.0f, w2 = 0.0f;
    if (se != 0.0f) {
        w0 = cv.e[0] / se;
        w1 = cv.e[1] / se;
        w2 = cv.e[2] / se;
    }
    float x, y;
    mesh_pixel_xy(cam, i, j, x, y);
    px.status = kRayHit | (p.det > 0.0f ? kRayFromBelow : 0);
    px.t = cv.depth * sqrtf((x * x + y * y) + 1.0f);
    float vpos[3];
    for (int k = 0; k < 3; ++k) {
        px.position[k] = (w0 * a.position[k] + w1 * b.position[k]) + w2 * c.position[k];
        vpos[k] = (w0 * a.view[k] + w1 * b.view[k]) + w2 * c.view[k];
    }
    px.p[0] = (w0 * a.uv[0] + w1 * b.uv[0]) + w2 * c.uv[0];
    px.p[1] = (w0 * a.uv[1] + w1 * b.uv[1]) + w2 * c.uv[1];
    const float wave_height = (w0 * a.wave_height + w1 * b.wave_height) + w2 * c.wave_height;
    const SurfaceSample s = sample_point(disp, norm, n, cascades, scales, px.p[0], px.p[1]);
    px.gradient_fragment[0] = s.gradient_fragment[0];
    px.gradient_fragment[1] = s.gradient_fragment[1];
    px.foam_fragment = s.foam_fragment;
    float rel[3], view[3];
    for (int k = 0; k < 3; ++k) rel[k] = px.position[k] - cam.o[k];
    const float len = sqrtf(dot3(rel, rel));
    for (int k = 0; k < 3; ++k) view[k] = len > 0.0f ? -rel[k] / len : (k == 1 ? 1.0f : 0.0f);
    const Fragment f = shade_fragment(sp, s, wave_height, vpos[0], vpos[2], view);
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
    px.reserved[0] = (uint32_t)tri + 1u;
    *rgba = pack_rgba8(px.color);
    return px;
}

}  // namespace ow

// mesh_harness.cpp -- godotoceanwaves_amd/csrc/ow_mesh.h compiled as plain C++ (g++ -ffp-contract=off): the vertex stage, the triangles
// taken in order against every pixel centre of their box with the same min the device's atomicMin takes, and the per-pixel record.
// Test infrastructure (tests/test_mesh_draw.py); the device's vertex records, visibility words, RGBA8 words and pixel records are held
// to these bit for bit.  With -DMESH_HARNESS_MAIN it is a stand-alone program that draws the calm-sea cameras and the awkward inputs of
// the test-suite on maps it makes itself and checks what every picture must hold: the form the sanitizers run.
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "ow_mesh.h"

namespace {

// camera: position[3], basis[9], tan(fov / 2), aspect, max_distance as the runtime resolves them from ow_camera
ow::CameraParams camera_of(const float *camera, int width, int height) {
    ow::CameraParams cam;
    memset(&cam, 0, sizeof(cam));
    if (camera) {
        memcpy(cam.o, camera, 3 * sizeof(float));
        memcpy(cam.B, camera + 3, 9 * sizeof(float));
        cam.tan_half_fov = camera[12];
        cam.aspect = camera[13];
        cam.max_distance = camera[14];
    }
    cam.width = width;
    cam.height = height;
    return cam;
}

ow::MeshParams params_of(int falloff, float cx, float cz, float near, int cull_back, int lane_box, const ow::CameraParams &cam, bool has_camera) {
    ow::MeshParams mp;
    mp.qp.max_iterations = ow::kQueryDefaultIterations;
    mp.qp.tolerance = ow::kQueryDefaultTolerance;
    mp.qp.falloff = falloff;
    mp.qp.center[0] = cx;
    mp.qp.center[1] = cz;
    mp.near = near > 0.0f ? near : ow::kMeshDefaultNear;
    mp.cull_back = cull_back;
    mp.lane_box = lane_box == 0 ? ow::kMeshLaneBox : (lane_box < 0 ? 0 : lane_box);
    mp.camera_ok = has_camera && ow::mesh_camera_ok(cam) ? 1 : 0;
    return mp;
}

ow::SurfaceScales scales_of(const float *map_scales, int cascades) {
    ow::SurfaceScales sc;
    memset(&sc, 0, sizeof(sc));
    memcpy(sc.s, map_scales, (size_t)cascades * 4 * sizeof(float));
    return sc;
}

// The draw in its two forms.  brute: the box is ignored (harness_mesh_cover_all below).  setups_out: five integers a triangle; cover_out:
// two (brute only).
void mesh_draw(const uint16_t *disp, const uint16_t *norm, int n, int cascades, const float *map_scales, const float *local, int num_vertices,
               const int32_t *indices, int num_triangles, const float *origin, const float *camera, int width, int height, const float *shade, int falloff,
               float cx, float cz, float near, int cull_back, int lane_box, ow::MeshVertex *vertices_out, uint64_t *vis_out, uint32_t *rgba,
               ow::RenderPixel *pixels, uint32_t *counters, bool brute, int32_t *setups_out, int32_t *cover_out) {
    static_assert(sizeof(ow::ShadeParams) == 22 * sizeof(float), "ShadeParams is 22 floats");
    const ow::SurfaceScales sc = scales_of(map_scales, cascades);
    const ow::CameraParams cam = camera_of(camera, width, height);
    const ow::MeshParams mp = params_of(falloff, cx, cz, near, cull_back, lane_box, cam, true);
    ow::ShadeParams sp;
    memcpy(&sp, shade, sizeof(sp));
    const ow::u16x4 *d = (const ow::u16x4 *)disp;
    std::vector<ow::MeshVertex> verts((size_t)num_vertices);
    for (int i = 0; i < num_vertices; ++i) verts[i] = ow::mesh_vertex(d, n, cascades, sc, mp, cam, true, local + 3 * (size_t)i, origin);
    std::vector<uint64_t> vis((size_t)width * height, ow::kMeshNoTriangle);
    uint32_t count[4] = {0, 0, 0, 0};
    for (int t = 0; t < num_triangles; ++t) {
        const ow::TriSetup s = ow::tri_setup(verts[indices[3 * (size_t)t]], verts[indices[3 * (size_t)t + 1]], verts[indices[3 * (size_t)t + 2]], cam, mp);
        ++count[s.kind];
        if (setups_out) {
            const int32_t five[5] = {s.kind, s.x0, s.x1, s.y0, s.y1};
            memcpy(setups_out + 5 * (size_t)t, five, sizeof(five));
        }
        const bool boxed = s.kind == ow::kTriLane || s.kind == ow::kTriWave;
        int x0 = s.x0, x1 = s.x1, y0 = s.y0, y1 = s.y1;
        if (brute) {  // what tri_setup culls before it looks at the box: flags, a camera that is not finite (both leave det 0), det, facing
            if (s.kind == ow::kTriSkipped || !(s.p.det != 0.0f) || (mp.cull_back && s.p.det > 0.0f)) continue;
            x0 = y0 = 0, x1 = width - 1, y1 = height - 1;
        } else if (!boxed) {
            continue;
        }
        int32_t covered = 0, outside = 0;
        for (int j = y0; j <= y1; ++j)
            for (int i = x0; i <= x1; ++i) {
                const ow::TriCover c = ow::tri_cover(s.p, cam, mp.near, i, j);
                if (!c.hit) continue;
                ++covered;
                outside += !(boxed && i >= s.x0 && i <= s.x1 && j >= s.y0 && j <= s.y1);
                const uint64_t w = ow::mesh_word(c.depth, t);
                uint64_t &at = vis[(size_t)j * width + i];
                if (w < at) at = w;
            }
        if (cover_out) cover_out[2 * (size_t)t] = covered, cover_out[2 * (size_t)t + 1] = outside;
    }
    for (int j = 0; j < height && (rgba || pixels); ++j)
        for (int i = 0; i < width; ++i) {
            const size_t at = (size_t)j * width + i;
            uint32_t word;
            const ow::RenderPixel px = ow::mesh_pixel(d, (const ow::u16x4 *)norm, n, cascades, sc, cam, sp, mp, vis[at], indices, verts.data(), i, j, &word);
            if (rgba) rgba[at] = word;
            if (pixels) pixels[at] = px;
        }
    if (vertices_out) memcpy(vertices_out, verts.data(), verts.size() * sizeof(ow::MeshVertex));
    if (vis_out) memcpy(vis_out, vis.data(), vis.size() * sizeof(uint64_t));
    if (counters) memcpy(counters, count, sizeof(count));
}

}  // namespace

extern "C" {

int harness_mesh_sizes(int *sizes) {
    sizes[0] = (int)sizeof(ow::MeshVertex);
    sizes[1] = (int)offsetof(ow::MeshVertex, wave_height);
    sizes[2] = (int)offsetof(ow::MeshVertex, uv);
    sizes[3] = (int)offsetof(ow::MeshVertex, falloff);
    sizes[4] = (int)offsetof(ow::MeshVertex, view);
    sizes[5] = (int)offsetof(ow::MeshVertex, flags);
    sizes[6] = (int)sizeof(ow::MeshParams);
    sizes[7] = (int)sizeof(ow::RenderPixel);
    return 0;
}

// the vertex stage: `count` local positions -> records; camera may be NULL (view positions are zeros then)
void harness_mesh_vertices(const uint16_t *disp, int n, int cascades, const float *map_scales, const float *local, int count, const float *origin,
                           int falloff, float cx, float cz, const float *camera, ow::MeshVertex *out) {
    const ow::SurfaceScales sc = scales_of(map_scales, cascades);
    const ow::CameraParams cam = camera_of(camera, 1, 1);
    const ow::MeshParams mp = params_of(falloff, cx, cz, 0.0f, 0, 0, cam, camera != NULL);
    for (int i = 0; i < count; ++i) out[i] = ow::mesh_vertex((const ow::u16x4 *)disp, n, cascades, sc, mp, cam, camera != NULL, local + 3 * (size_t)i, origin);
}

// The whole draw.  shade: the 22 floats of ow::ShadeParams.  vertices_out (num_vertices records), vis_out (width * height words), rgba,
// pixels and counters (4 words: skipped, culled, per lane, by the wave) may each be NULL.
void harness_mesh_draw(const uint16_t *disp, const uint16_t *norm, int n, int cascades, const float *map_scales, const float *local, int num_vertices,
                       const int32_t *indices, int num_triangles, const float *origin, const float *camera, int width, int height, const float *shade,
                       int falloff, float cx, float cz, float near, int cull_back, int lane_box, ow::MeshVertex *vertices_out, uint64_t *vis_out,
                       uint32_t *rgba, ow::RenderPixel *pixels, uint32_t *counters) {
    mesh_draw(disp, norm, n, cascades, map_scales, local, num_vertices, indices, num_triangles, origin, camera, width, height, shade, falloff, cx, cz, near,
              cull_back, lane_box, vertices_out, vis_out, rgba, pixels, counters, false, NULL, NULL);
}

// The same draw without the walk's box: every triangle that its vertices' flags, det == 0 and the facing do not cull is tested with
// tri_cover at every centre of the picture, whatever tri_setup made of its box (!any, all_far and an empty box included), and the words
// are combined with the same min.  The reference tests/test_raster_edges.py holds the boxed draw and the device to.  The counters are the
// set-ups' classes, as the draw counts them.  cover_out (may be NULL): per triangle, the centres it covers and how many of them lie
// outside its set-up's box (a class that is not drawn has no box).
void harness_mesh_cover_all(const uint16_t *disp, const uint16_t *norm, int n, int cascades, const float *map_scales, const float *local, int num_vertices,
                            const int32_t *indices, int num_triangles, const float *origin, const float *camera, int width, int height,
                            const float *shade, int falloff, float cx, float cz, float near, int cull_back, int lane_box, ow::MeshVertex *vertices_out,
                            uint64_t *vis_out, uint32_t *rgba, ow::RenderPixel *pixels, uint32_t *counters, int32_t *cover_out) {
    mesh_draw(disp, norm, n, cascades, map_scales, local, num_vertices, indices, num_triangles, origin, camera, width, height, shade, falloff, cx, cz, near,
              cull_back, lane_box, vertices_out, vis_out, rgba, pixels, counters, true, NULL, cover_out);
}

// every triangle's set-up as the draw makes it: kind, x0, x1, y0, y1
void harness_mesh_setups(const uint16_t *disp, const uint16_t *norm, int n, int cascades, const float *map_scales, const float *local, int num_vertices,
                         const int32_t *indices, int num_triangles, const float *origin, const float *camera, int width, int height, const float *shade,
                         int falloff, float cx, float cz, float near, int cull_back, int lane_box, int32_t *setups_out) {
    mesh_draw(disp, norm, n, cascades, map_scales, local, num_vertices, indices, num_triangles, origin, camera, width, height, shade, falloff, cx, cz, near,
              cull_back, lane_box, NULL, NULL, NULL, NULL, NULL, false, setups_out, NULL);
}

}  // extern "C"

#ifdef MESH_HARNESS_MAIN
// ---- the stand-alone form ---------------------------------------------------------------------------------------------------------------
namespace {

int g_failures = 0;
#define EXPECT(cond, what)                                                  \
    do {                                                                    \
        if (!(cond)) {                                                      \
            ++g_failures;                                                   \
            fprintf(stderr, "FAILED %s: %s (line %d)\n", what, #cond, __LINE__); \
        }                                                                   \
    } while (0)

struct Maps {
    int n, cascades;
    std::vector<uint16_t> disp, norm;
    std::vector<float> scales;
};
Maps calm_maps() {
    Maps m;
    m.n = 64;
    m.cascades = 2;
    m.disp.assign((size_t)2 * 64 * 64 * 4, 0);
    m.norm.assign((size_t)2 * 64 * 64 * 4, 0);
    m.scales = {1 / 50.0f, 1 / 50.0f, 1.0f, 1.0f, 1 / 50.0f, 1 / 50.0f, 1.0f, 1.0f};
    return m;
}
// a choppy swell: D = (-A sin(k x), A cos(k x), 0.3 A sin(k z)) at the texel centres, gradients to match, foam in .w
Maps swell_maps(float displacement_scale) {
    Maps m;
    m.n = 128;
    m.cascades = 1;
    const float tile = 40.0f, A = 0.8f, k = 2.0f * 3.14159265f / 10.0f;
    m.disp.resize((size_t)m.n * m.n * 4);
    m.norm.resize((size_t)m.n * m.n * 4);
    for (int r = 0; r < m.n; ++r)
        for (int c = 0; c < m.n; ++c) {
            const float x = (c + 0.5f) * tile / m.n, z = (r + 0.5f) * tile / m.n;
            uint16_t *d = &m.disp[((size_t)r * m.n + c) * 4], *g = &m.norm[((size_t)r * m.n + c) * 4];
            d[0] = ow::f2h(-A * sinf(k * x));
            d[1] = ow::f2h(A * cosf(k * x));
            d[2] = ow::f2h(0.3f * A * sinf(k * z));
            d[3] = 0;
            g[0] = ow::f2h(-A * k * sinf(k * x));
            g[1] = ow::f2h(0.1f * cosf(k * z));
            g[2] = 0;
            g[3] = ow::f2h(0.5f + 0.5f * sinf(k * x));
        }
    m.scales = {1 / tile, 1 / tile, displacement_scale, 1.0f};
    return m;
}

struct Mesh {
    std::vector<float> v;
    std::vector<int32_t> t;
};
Mesh grid(int cells, float cell) {
    Mesh m;
    const float half = 0.5f * cells * cell;
    for (int r = 0; r <= cells; ++r)
        for (int c = 0; c <= cells; ++c) {
            m.v.push_back(c * cell - half);
            m.v.push_back(0.0f);
            m.v.push_back(r * cell - half);
        }
    for (int r = 0; r < cells; ++r)
        for (int c = 0; c < cells; ++c) {
            const int a = r * (cells + 1) + c, b = a + 1, d = a + cells + 1, e = d + 1;
            const int32_t tri[6] = {a, d, b, b, d, e};  // counter-clockwise seen from above
            m.t.insert(m.t.end(), tri, tri + 6);
        }
    return m;
}

// position, yaw (0 = +z), pitch (negative = down): the 15 camera words
std::vector<float> look(float px, float py, float pz, double yaw_deg, double pitch_deg, double fov, int width, int height, float max_distance) {
    const double yaw = yaw_deg * 3.14159265358979323846 / 180.0, pitch = pitch_deg * 3.14159265358979323846 / 180.0;
    const double f[3] = {sin(yaw) * cos(pitch), sin(pitch), cos(yaw) * cos(pitch)};
    double r[3] = {f[1] * 0.0 - f[2] * 1.0, f[2] * 0.0 - f[0] * 0.0, f[0] * 1.0 - f[1] * 0.0};   // f x (0, 1, 0)
    const double rl = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    for (double &x : r) x /= rl;
    const double u[3] = {r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]};
    std::vector<float> w = {px, py, pz};
    for (int k = 0; k < 3; ++k) {  // rows of the basis: columns right, up, back
        w.push_back((float)r[k]);
        w.push_back((float)u[k]);
        w.push_back((float)-f[k]);
    }
    w.push_back((float)tan(fov * 3.14159265358979323846 / 360.0));
    w.push_back((float)width / (float)height);
    w.push_back(max_distance);
    return w;
}

const float kShade[22] = {0.0100228256f, 0.019606648f, 0.0272117816f, 0.491905034f, 0.406448305f, 0.34239164f, 0.65f, 1.0f, 0.87f, 12.9f,
                          0.321197f, 0.18296f, 0.929171f, 1.0f, 1.0f, 1.0f, 0.05f, 0.08f, 0.10f, 0.25f, 0.40f, 0.60f};

struct Picture {
    int width, height;
    std::vector<uint64_t> vis;
    std::vector<uint32_t> rgba;
    std::vector<ow::RenderPixel> px;
    uint32_t count[4];
    int hits;
};
Picture draw(const char *what, const Maps &maps, const Mesh &mesh, const std::vector<float> &cam, int width, int height, int cull_back, int falloff) {
    Picture p;
    p.width = width;
    p.height = height;
    p.vis.resize((size_t)width * height);
    p.rgba.resize((size_t)width * height);
    p.px.resize((size_t)width * height);
    const float origin[3] = {0.0f, 0.0f, 0.0f};
    std::vector<ow::MeshVertex> verts(mesh.v.size() / 3);
    harness_mesh_draw(maps.disp.data(), maps.norm.data(), maps.n, maps.cascades, maps.scales.data(), mesh.v.data(), (int)(mesh.v.size() / 3), mesh.t.data(),
                      (int)(mesh.t.size() / 3), origin, cam.data(), width, height, kShade, falloff, cam[0], cam[2], 0.0f, cull_back, 0, verts.data(),
                      p.vis.data(), p.rgba.data(), p.px.data(), p.count);
    p.hits = 0;
    EXPECT(p.count[0] + p.count[1] + p.count[2] + p.count[3] == mesh.t.size() / 3, what);
    for (size_t i = 0; i < p.px.size(); ++i) {
        const ow::RenderPixel &r = p.px[i];
        const float *f = &r.t;
        bool finite = true;
        for (int k = 0; k < 28; ++k)
            if (k != 1) finite = finite && isfinite(f[k]);
        EXPECT(finite, what);
        const bool hit = (r.status & ow::kRayHit) != 0;
        EXPECT(hit == (p.vis[i] != ow::kMeshNoTriangle), what);
        EXPECT(hit ? r.reserved[0] == (uint32_t)p.vis[i] + 1u : r.reserved[0] == 0u, what);
        if (!hit) EXPECT(r.t == 0.0f && r.color[0] == kShade[19] && r.color[1] == kShade[20] && r.color[2] == kShade[21], what);
        EXPECT((p.rgba[i] >> 24) == 255u, what);
        p.hits += hit;
    }
    printf("%-44s %4d x %-4d hits %6d  skipped %u culled %u lane %u wave %u\n", what, width, height, p.hits, p.count[0], p.count[1], p.count[2], p.count[3]);
    return p;
}

}  // namespace

int main() {
    const Maps calm = calm_maps();
    const Mesh g = grid(16, 4.0f);   // 17 x 17 vertices, 4 m cells: the square |x|, |z| <= 32
    // the calm sea's three cameras: every ray that meets y = 0 inside the square within (near, far] is covered, and nothing else
    struct Cam {
        const char *what;
        float p[3];
        double yaw, pitch;
    } cams[3] = {{"calm sea, straight down", {1.0f, 20.0f, -2.0f}, 0.0, -89.9}, {"calm sea, pitched -25 from 12 m", {0.0f, 12.0f, -20.0f}, 10.0, -25.0},
                 {"calm sea, 0.5 m up, level", {0.3f, 0.5f, 0.2f}, 30.0, 0.0}};
    for (const Cam &c : cams) {
        const std::vector<float> cam = look(c.p[0], c.p[1], c.p[2], c.yaw, c.pitch, 75.0, 64, 40, 200.0f);
        const Picture p = draw(c.what, calm, g, cam, 64, 40, 0, 0);
        const ow::CameraParams cp = camera_of(cam.data(), 64, 40);
        for (int j = 0; j < 40; ++j)
            for (int i = 0; i < 64; ++i) {
                const ow::Ray r = ow::pixel_ray(cp, i, j);
                const double dy = r.direction[1];
                bool want = false;
                double margin = 0.0;
                if (dy < 0.0) {
                    const double s = -(double)c.p[1] / dy, x = c.p[0] + s * r.direction[0], z = c.p[2] + s * r.direction[2];   // s: the view depth
                    margin = fmin(fmin(32.0 - fabs(x), 32.0 - fabs(z)), fmin(s - 0.05, 200.0 - s));
                    want = margin > 0.0;
                }
                const bool hit = (p.px[(size_t)j * 64 + i].status & ow::kRayHit) != 0;
                if (fabs(margin) > 1e-3 || dy >= 0.0) EXPECT(hit == want, c.what);
                if (hit) EXPECT(fabs(p.px[(size_t)j * 64 + i].position[1]) <= 1e-4f, c.what);
            }
        EXPECT(p.hits > 0, c.what);
    }
    // the awkward inputs
    const Maps swell = swell_maps(1.0f), folded = swell_maps(4.0f);
    const std::vector<float> over = look(0.0f, 12.0f, -20.0f, 10.0, -25.0, 75.0, 37, 21, 500.0f);
    {
        Mesh one;
        one.v = {-5, 0, -5, 5, 0, 5, 5, 0, -5};
        one.t = {0, 1, 2};
        EXPECT(draw("one triangle", swell, one, over, 37, 21, 0, 1).hits > 0, "one triangle");
        Mesh flat = one;
        flat.v.insert(flat.v.end(), {0, 0, 0});
        flat.t = {0, 3, 1, 0, 0, 1, 2, 2, 2, 0, 1, 2};   // collinear, two equal corners, three equal corners, and a real one
        EXPECT(draw("zero-area triangles", calm, flat, over, 37, 21, 0, 0).hits > 0, "zero-area triangles");
        Mesh huge;
        huge.v = {-1e4f, 0, -1e4f, 0, 0, 2e4f, 1e4f, 0, -1e4f};
        huge.t = {0, 1, 2};
        const Picture p = draw("a triangle larger than the screen", calm, huge, look(0.0f, 12.0f, -20.0f, 10.0, -60.0, 40.0, 37, 21, 500.0f), 37, 21, 0, 0);
        EXPECT(p.hits == 37 * 21 && p.count[3] == 1, "a triangle larger than the screen");
        Mesh nan = g;
        nan.v[3 * 40 + 1] = NAN;
        nan.v[3 * 100] = INFINITY;
        const Picture q = draw("two vertices that are not finite", swell, nan, over, 37, 21, 0, 0);
        EXPECT(q.count[0] > 0 && q.count[0] <= 12, "two vertices that are not finite");
    }
    EXPECT(draw("wholly behind the camera", swell, g, look(0.0f, 5.0f, 60.0f, 0.0, -10.0, 75.0, 37, 21, 500.0f), 37, 21, 0, 0).hits == 0, "behind");
    EXPECT(draw("wholly off-screen", swell, g, look(0.0f, 5.0f, -60.0f, 120.0, 0.0, 40.0, 37, 21, 500.0f), 37, 21, 0, 0).hits == 0, "off-screen");
    {
        const Picture p = draw("sub-pixel triangles", swell, grid(128, 0.5f), look(0.0f, 60.0f, -150.0f, 0.0, -20.0, 75.0, 37, 21, 500.0f), 37, 21, 0, 1);
        EXPECT(p.hits > 0 && p.count[2] > p.count[3], "sub-pixel triangles");
    }
    EXPECT(draw("a folded mesh", folded, grid(64, 0.5f), over, 37, 21, 0, 0).hits > 0, "a folded mesh");
    {
        const std::vector<float> below = look(0.0f, -6.0f, -10.0f, 0.0, 30.0, 75.0, 37, 21, 500.0f);
        const Picture p = draw("from below", swell, g, below, 37, 21, 0, 0);
        bool all_below = p.hits > 0;
        for (const ow::RenderPixel &r : p.px)
            if (r.status & ow::kRayHit) all_below = all_below && (r.status & ow::kRayFromBelow);
        EXPECT(all_below, "from below");
        EXPECT(draw("calm sea from below", calm, g, below, 37, 21, 0, 0).hits > 0, "calm sea from below");
        EXPECT(draw("calm sea from below, back faces culled", calm, g, below, 37, 21, 1, 0).hits == 0, "calm sea from below, back faces culled");
        draw("from below, back faces culled", swell, g, below, 37, 21, 1, 0);   // a steep crest may still show its upper side
    }
    draw("a 1 x 1 image", swell, g, look(0.0f, 12.0f, -20.0f, 10.0, -25.0, 75.0, 1, 1, 500.0f), 1, 1, 0, 0);
    {
        std::vector<float> bad = over;
        bad[1] = NAN;
        const Picture p = draw("a camera that is not finite", swell, g, bad, 37, 21, 0, 0);
        bool all_invalid = p.hits == 0;
        for (const ow::RenderPixel &r : p.px) all_invalid = all_invalid && r.status == ow::kRayInvalid;
        EXPECT(all_invalid, "a camera that is not finite");
    }
    {   // one soup through both forms: a camera at the origin with the identity basis over zero maps, so a local position is a view
        // position; triangles in front at any size, across the near plane and around the camera; the boxed draw is the brute one
        const std::vector<float> eye = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1.0f, 37.0f / 21.0f, 200.0f};
        Mesh soup;
        uint32_t lcg = 20261021u;
        auto next = [&lcg]() { return (float)((lcg = lcg * 1664525u + 1013904223u) >> 8) / 16777216.0f; };
        for (int t = 0; t < 600; ++t) {
            const float z = t % 3 == 0 ? 0.0f : -(0.06f + 40.0f * next() * next()), spread = t % 3 == 2 ? 0.1f : 3.0f * (0.05f - z) * next();
            const float c[3] = {(2.0f * next() - 1.0f) * (1.0f - z), (2.0f * next() - 1.0f) * (1.0f - z), z};
            for (int k = 0; k < 3; ++k) {
                for (int a = 0; a < 3; ++a) soup.v.push_back(c[a] + (2.0f * next() - 1.0f) * (t % 3 == 0 ? 2.0f : spread));
                soup.t.push_back(3 * t + k);
            }
        }
        const float origin[3] = {0.0f, 0.0f, 0.0f};
        const int nt = (int)(soup.t.size() / 3), nv = (int)(soup.v.size() / 3);
        for (int lane_box : {0, -1, 1, 64}) {
            std::vector<uint64_t> boxed(37 * 21), brute(37 * 21);
            std::vector<int32_t> setups(5 * (size_t)nt), cover(2 * (size_t)nt, 0);
            uint32_t cb[4], ca[4];
            harness_mesh_draw(calm.disp.data(), calm.norm.data(), calm.n, calm.cascades, calm.scales.data(), soup.v.data(), nv, soup.t.data(), nt, origin,
                              eye.data(), 37, 21, kShade, 0, 0.0f, 0.0f, 0.0f, 0, lane_box, NULL, boxed.data(), NULL, NULL, cb);
            harness_mesh_cover_all(calm.disp.data(), calm.norm.data(), calm.n, calm.cascades, calm.scales.data(), soup.v.data(), nv, soup.t.data(), nt, origin,
                                   eye.data(), 37, 21, kShade, 0, 0.0f, 0.0f, 0.0f, 0, lane_box, NULL, brute.data(), NULL, NULL, ca, cover.data());
            harness_mesh_setups(calm.disp.data(), calm.norm.data(), calm.n, calm.cascades, calm.scales.data(), soup.v.data(), nv, soup.t.data(), nt, origin,
                                eye.data(), 37, 21, kShade, 0, 0.0f, 0.0f, 0.0f, 0, lane_box, setups.data());
            EXPECT(boxed == brute && memcmp(cb, ca, sizeof(cb)) == 0, "a soup: boxed and brute");
            int outside = 0, covered = 0, drawn = 0;
            for (int t = 0; t < nt; ++t) {
                covered += cover[2 * (size_t)t];
                outside += cover[2 * (size_t)t + 1];
                drawn += setups[5 * (size_t)t] >= 2;
            }
            EXPECT(outside == 0 && covered > 0 && drawn == (int)(cb[2] + cb[3]), "a soup: no covered centre outside a box");
            printf("%-44s lane_box %2d  covered %d  lane %u wave %u\n", "a soup, boxed and brute", lane_box, covered, cb[2], cb[3]);
        }
    }
    printf("%s (%d failures)\n", g_failures ? "FAILED" : "ok", g_failures);
    return g_failures ? 1 : 0;
}
#endif

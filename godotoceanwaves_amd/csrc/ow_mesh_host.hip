// ow_mesh_host.hip -- the displaced water mesh: the ow_mesh_* handles, ow_mesh_displace and ow_mesh_draw in both forms, over the kernels
// of ow_mesh.hip (ow_mesh.h).  Its material is ow_render_options' (resolve_render_options), field for field.
#include <cmath>
#include <cstring>

#include "ow_consumer_host.h"

using namespace ow::readside;
using ow::fail, ow::layer_mask, ow::main_stream, ow::sync_stream;

namespace {
// the eight material fields ow_render_options and ow_mesh_options share
template <class To, class From>
void copy_material(To *to, const From &from) {
    for (int k = 0; k < 3; ++k) {
        to->water_color[k] = from.water_color[k];
        to->foam_color[k] = from.foam_color[k];
        to->light_direction[k] = from.light_direction[k];
        to->light_color[k] = from.light_color[k];
        to->ambient_color[k] = from.ambient_color[k];
        to->sky_color[k] = from.sky_color[k];
    }
    to->roughness = from.roughness;
    to->normal_strength = from.normal_strength;
}

// ow_mesh_options (NULL = the defaults) -> the draw's settings and the shading's: the shared fields go through resolve_render_options
ow_status resolve_mesh_options(const ow_mesh_options *opts, ow::MeshParams *mp, ow::ShadeParams *sp) {
    static_assert(sizeof(ow_mesh_vertex) == sizeof(ow::MeshVertex) && offsetof(ow_mesh_vertex, uv) == offsetof(ow::MeshVertex, uv) &&
                      offsetof(ow_mesh_vertex, distance_factor) == offsetof(ow::MeshVertex, falloff) &&
                      offsetof(ow_mesh_vertex, view_position) == offsetof(ow::MeshVertex, view) &&
                      offsetof(ow_mesh_vertex, flags) == offsetof(ow::MeshVertex, flags) && OW_MESH_VERTEX_NOT_FINITE == ow::kMeshVertexNotFinite,
                  "record layout");
    ow_render_options ro;
    render_defaults(&ro);
    ow_query_options qo;
    std::memset(&qo, 0, sizeof(qo));
    mp->near = ow::kMeshDefaultNear;
    mp->cull_back = 0;
    mp->lane_box = ow::kMeshLaneBox;
    mp->camera_ok = 1;
    if (opts) {
        copy_material(&ro, *opts);
        qo.flags = opts->query_flags;
        qo.falloff_center_xz[0] = opts->falloff_center_xz[0];
        qo.falloff_center_xz[1] = opts->falloff_center_xz[1];
    }
    ow::RaycastParams unused;
    if (ow_status st = resolve_render_options(&ro, &unused, sp); st != OW_OK) return st;
    if (ow_status st = ow::resolve_query_options(&qo, &mp->qp); st != OW_OK) return st;
    if (!opts) return OW_OK;
    if (!std::isfinite(opts->near)) return fail(OW_ERR_INVALID, "near is not finite");
    if (opts->flags & ~OW_MESH_CULL_BACK) return fail(OW_ERR_INVALID, "unknown mesh flags 0x%x", opts->flags);
    if (ow_status st = resolve_lane_box(opts->lane_box, &mp->lane_box); st != OW_OK) return st;
    if (ow_status st = check_reserved(opts->reserved, "ow_mesh_options"); st != OW_OK) return st;
    if (opts->near > 0.0f) mp->near = opts->near;
    mp->cull_back = (opts->flags & OW_MESH_CULL_BACK) ? 1 : 0;
    return OW_OK;
}

ow_status check_mesh_handle(const ow_context *c, const ow_mesh *m) { return check_handle(c, m, "mesh"); }

// the argument checks both forms of ow_mesh_draw share: ow_render_view's, in its order, then the mesh and the origin
ow_status check_mesh_draw(const ow_context *c, const ow_mesh *m, const ow_camera *camera, const float *origin, const float *map_scales,
                          int32_t num_cascades, const ow_mesh_options *opts, const void *rgba, const void *pixels, ow::CameraParams *cp,
                          ow::MeshParams *mp, ow::ShadeParams *sp) {
    if (!rgba && !pixels) return fail(OW_ERR_INVALID, "null argument: both outputs");
    if (!map_scales) return fail(OW_ERR_INVALID, "null argument");
    if (ow_status st = resolve_camera(camera, cp); st != OW_OK) return st;
    if (ow_status st = resolve_mesh_options(opts, mp, sp); st != OW_OK) return st;
    if (ow_status st = check_point_query(c, 0, num_cascades); st != OW_OK) return st;
    if (ow_status st = check_mesh_handle(c, m); st != OW_OK) return st;
    if (!origin) return fail(OW_ERR_INVALID, "null origin");
    mp->camera_ok = ow::mesh_camera_ok(*cp) ? 1 : 0;
    return OW_OK;
}

// the visibility words of a draw of `count` pixels (exact size)
ow_status mesh_vis_scratch(ow_context *c, size_t count) {
    if (ow_status st = sync_before_growth(c, c->mesh_vis, count * sizeof(uint64_t)); st != OW_OK) return st;
    return c->mesh_vis.ensure(count * sizeof(uint64_t), 0, sizeof(uint64_t), "visibility words");
}
// a draw's launch on the context's stream (the visibility words are there: mesh_vis_scratch)
ow_status mesh_enqueue(ow_context *c, ow_mesh *m, const ow::CameraParams &cp, const float *origin, const float *map_scales, int num_cascades,
                       const ow::MeshParams &mp, const ow::ShadeParams &sp, uint32_t *rgba_dev, ow::RenderPixel *pixels_dev) {
    const ow::MapsView v = view_of(c);
    OW_HIP(ow::launch_mesh_draw(v.n, num_cascades, v.buf, m->A, surface_scales(map_scales, num_cascades), mp, cp, sp, origin, (uint64_t *)c->mesh_vis.ptr, rgba_dev,
                                pixels_dev, v.stream));
    ++m->draws;
    return OW_OK;
}
}  // namespace

extern "C" {

void ow_mesh_options_default(ow_mesh_options *out) {
    if (!out) return;
    ow_render_options ro;
    render_defaults(&ro);
    std::memset(out, 0, sizeof(*out));
    copy_material(out, ro);
    out->near = ow::kMeshDefaultNear;
}

ow_status ow_mesh_create(ow_context *c, const float *vertices_xyz, int32_t num_vertices, const int32_t *indices, int32_t num_triangles, ow_mesh **out) {
    if (!out) return fail(OW_ERR_INVALID, "null argument");
    *out = nullptr;
    if (num_vertices < 1 || num_triangles < 1) return fail(OW_ERR_INVALID, "num_vertices and num_triangles must be >= 1");
    if (!vertices_xyz || !indices) return fail(OW_ERR_INVALID, "null argument");
    for (size_t i = 0; i < (size_t)num_triangles * 3; ++i)
        if (indices[i] < 0 || indices[i] >= num_vertices)
            return fail(OW_ERR_INVALID, "triangle %zu: index %d outside [0,%d)", i / 3, indices[i], num_vertices);
    if (!c) return fail(OW_ERR_INVALID, "null context");
    const size_t nv = (size_t)num_vertices, nt = (size_t)num_triangles;
    Layout L;
    const size_t l_off = L.take(nv * 3 * sizeof(float)), i_off = L.take(nt * 3 * sizeof(int32_t)), v_off = L.take(nv * sizeof(ow::MeshVertex));
    const size_t c_off = L.take(4 * sizeof(uint32_t));  // kTriSkipped .. kTriWave
    ow_mesh *m;
    if (ow_status st = new_handle(c, L.total, "mesh", &m); st != OW_OK) return st;
    char *base = (char *)m->block;
    m->A.local = (const float *)(base + l_off);
    m->A.indices = (const int32_t *)(base + i_off);
    m->A.verts = (ow::MeshVertex *)(base + v_off);
    m->A.counters = (uint32_t *)(base + c_off);
    m->A.num_vertices = num_vertices;
    m->A.num_triangles = num_triangles;
    hipStream_t s = main_stream(c);
    const bool enqueued = hipMemsetAsync(m->block, 0, L.total, s) == hipSuccess &&
                          hipMemcpyAsync((void *)m->A.local, vertices_xyz, nv * 3 * sizeof(float), hipMemcpyHostToDevice, s) == hipSuccess &&
                          hipMemcpyAsync((void *)m->A.indices, indices, nt * 3 * sizeof(int32_t), hipMemcpyHostToDevice, s) == hipSuccess;
    return finish_create(c, m, s, enqueued, "mesh upload", out);
}

void ow_mesh_destroy(ow_context *, ow_mesh *m) {
    if (m) release_handle(m);
    delete m;
}

ow_status ow_mesh_displace(ow_context *c, ow_mesh *m, const float *origin, const float *map_scales, int32_t num_cascades, const ow_mesh_options *opts,
                           const ow_camera *camera, ow_mesh_vertex *vertices_out) {
    if (!map_scales) return fail(OW_ERR_INVALID, "null argument");
    ow::CameraParams cp;
    std::memset(&cp, 0, sizeof(cp));
    if (camera) {
        ow_camera sized = *camera;  // the image size is not read here
        sized.width = sized.height = 1;
        if (ow_status st = resolve_camera(&sized, &cp); st != OW_OK) return st;
    }
    ow::MeshParams mp;
    ow::ShadeParams sp;
    if (ow_status st = resolve_mesh_options(opts, &mp, &sp); st != OW_OK) return st;
    if (ow_status st = check_point_query(c, 0, num_cascades); st != OW_OK) return st;
    if (ow_status st = check_mesh_handle(c, m); st != OW_OK) return st;
    if (!origin) return fail(OW_ERR_INVALID, "null origin");
    mp.camera_ok = camera && ow::mesh_camera_ok(cp) ? 1 : 0;  // a camera that is not finite: view positions are zeros, as without one
    OW_HIP(hipSetDevice(c->device));
    OW_HIP(ow::launch_mesh_vertices(c->n, num_cascades, c->buf, m->A, surface_scales(map_scales, num_cascades), mp, cp, camera != nullptr, origin, main_stream(c)));
    if (vertices_out)
        OW_HIP(hipMemcpyAsync(vertices_out, m->A.verts, (size_t)m->A.num_vertices * sizeof(ow::MeshVertex), hipMemcpyDeviceToHost, main_stream(c)));
    return sync_stream(c, layer_mask(num_cascades));
}

ow_status ow_mesh_get_device_ptrs(ow_context *c, ow_mesh *m, void **vertices_dev, void **visibility_dev) {
    if (ow_status st = check_mesh_handle(c, m); st != OW_OK) return st;
    if (vertices_dev) *vertices_dev = m->A.verts;
    if (visibility_dev) *visibility_dev = c->mesh_vis.ptr;
    return OW_OK;
}

ow_status ow_mesh_draw(ow_context *c, ow_mesh *m, const ow_camera *camera, const float *origin, const float *map_scales, int32_t num_cascades,
                       const ow_mesh_options *opts, void *rgba8_out, ow_render_pixel *pixels_out) {
    ow::CameraParams cp;
    ow::MeshParams mp;
    ow::ShadeParams sp;
    if (ow_status st = check_mesh_draw(c, m, camera, origin, map_scales, num_cascades, opts, rgba8_out, pixels_out, &cp, &mp, &sp); st != OW_OK) return st;
    OW_HIP(hipSetDevice(c->device));
    const size_t count = (size_t)cp.width * cp.height;
    if (ow_status st = mesh_vis_scratch(c, count); st != OW_OK) return st;
    return picture_round_trip(c, count, rgba8_out, pixels_out, false, layer_mask(num_cascades), [&](uint32_t *rgba_dev, ow::RenderPixel *px_dev) {
        return mesh_enqueue(c, m, cp, origin, map_scales, num_cascades, mp, sp, rgba_dev, px_dev);
    });
}

ow_status ow_mesh_draw_async(ow_context *c, ow_mesh *m, const ow_camera *camera, const float *origin, const float *map_scales, int32_t num_cascades,
                             const ow_mesh_options *opts, void *rgba8_dev, ow_render_pixel *pixels_dev) {
    ow::CameraParams cp;
    ow::MeshParams mp;
    ow::ShadeParams sp;
    if (ow_status st = check_mesh_draw(c, m, camera, origin, map_scales, num_cascades, opts, rgba8_dev, pixels_dev, &cp, &mp, &sp); st != OW_OK) return st;
    if (ow_status st = check_pixel_alignment(rgba8_dev, pixels_dev); st != OW_OK) return st;
    if (ow_status st = begin_async(c, num_cascades); st != OW_OK) return st;
    if (ow_status st = mesh_vis_scratch(c, (size_t)cp.width * cp.height); st != OW_OK) return st;
    return mesh_enqueue(c, m, cp, origin, map_scales, num_cascades, mp, sp, (uint32_t *)rgba8_dev, (ow::RenderPixel *)pixels_dev);
}

ow_status ow_mesh_stats(ow_context *c, ow_mesh *m, uint64_t *draws, uint64_t *skipped, uint64_t *culled, uint64_t *per_lane, uint64_t *cooperative) {
    if (ow_status st = check_mesh_handle(c, m); st != OW_OK) return st;
    uint64_t n[4];
    if (ow_status st = read_class_counts(c, m->A.counters, skipped || culled || per_lane || cooperative, n); st != OW_OK) return st;
    if (skipped) *skipped = n[ow::kTriSkipped];
    if (culled) *culled = n[ow::kTriCulled];
    if (per_lane) *per_lane = n[ow::kTriLane];
    if (cooperative) *cooperative = n[ow::kTriWave];
    if (draws) *draws = m->draws;
    return OW_OK;
}

}  // extern "C"

// ow_solid_host.hip -- the floating bodies as solids: the ow_solid_* shapes and draws over the kernels of ow_solid.hip (ow_solid.h), the
// ray casts against them, ow_cast_*, over those of ow_solid_cast.hip (ow_solid_cast.h), and their sun shadows, the ow_shadow_*
// maps, casts and pass, over those of ow_shadow.hip (ow_shadow.h).  A draw, a ray cast and a shadow cast take their instances from the same
// source (instance_source).
#include <cmath>
#include <cstring>

#include "ow_consumer_host.h"

using namespace ow::readside;
using ow::fail, ow::main_stream, ow::sync_stream;

/* ---- the solids (ow_solid.h, ow_solid.hip) ---- */

namespace {
// the reference scene's sun and ambient (ow_render_options_default), near 0.05, a wooden brown
void solid_defaults(ow_solid_options *o) {
    ow_render_options ro;
    render_defaults(&ro);
    std::memset(o, 0, sizeof(*o));
    const float color[3] = {0.45f, 0.30f, 0.15f};
    for (int k = 0; k < 3; ++k) {
        o->color[k] = color[k];
        o->light_direction[k] = ro.light_direction[k];
        o->light_color[k] = ro.light_color[k];
        o->ambient_color[k] = ro.ambient_color[k];
    }
    o->near = ow::kMeshDefaultNear;
}

// ow_solid_options (NULL = the defaults) -> the draw's constants
ow_status resolve_solid_options(const ow_solid_options *opts, ow::SolidParams *sp) {
    static_assert(sizeof(ow_solid_options) == sizeof(ow::SolidOptions) && offsetof(ow_solid_options, flags) == offsetof(ow::SolidOptions, flags) &&
                      offsetof(ow_solid_options, background_color) == offsetof(ow::SolidOptions, background_color) &&
                      offsetof(ow_solid_options, lane_box) == offsetof(ow::SolidOptions, lane_box) &&
                      offsetof(ow_solid_options, reserved) == offsetof(ow::SolidOptions, reserved) && OW_RAY_SOLID == ow::kRaySolid &&
                      OW_SOLID_TWO_SIDED == ow::kSolidTwoSided && OW_SOLID_MAX_INSTANCES == ow::kSolidMaxInstances &&
                      OW_SOLID_MAX_TRIANGLES == ow::kSolidMaxTriangles && sizeof(ow_buoyancy_body) % sizeof(float) == 0 &&
                      offsetof(ow_buoyancy_body, transform) == 0,
                  "record layout");
    ow_solid_options def;
    opts = or_defaults(opts, &def, solid_defaults);
    std::memset(sp, 0, sizeof(*sp));
    const float *vec[5] = {opts->color, opts->light_direction, opts->light_color, opts->ambient_color, opts->background_color};
    for (const float *v : vec)
        for (int k = 0; k < 3; ++k)
            if (!(std::fabs(v[k]) <= ow::kSolidColorMax)) return fail(OW_ERR_INVALID, "ow_solid_options: a colour or the light direction is not finite (or beyond 1e12)");
    if (!std::isfinite(opts->near)) return fail(OW_ERR_INVALID, "near is not finite");
    if (ow_status st = resolve_lane_box(opts->lane_box, &sp->mp.lane_box); st != OW_OK) return st;
    if (opts->flags & ~OW_SOLID_TWO_SIDED) return fail(OW_ERR_INVALID, "unknown solid flags 0x%x", opts->flags);
    if (ow_status st = check_reserved(opts->reserved, "ow_solid_options"); st != OW_OK) return st;
    const double lx = opts->light_direction[0], ly = opts->light_direction[1], lz = opts->light_direction[2];
    const double len = std::sqrt(lx * lx + ly * ly + lz * lz);
    if (!(len > 0.0)) return fail(OW_ERR_INVALID, "light_direction has zero length");
    for (int k = 0; k < 3; ++k) {
        sp->albedo[k] = opts->color[k];
        sp->light[k] = (float)((double)opts->light_direction[k] / len);
        sp->light_color[k] = opts->light_color[k];
        sp->ambient_color[k] = opts->ambient_color[k];
        sp->background[k] = opts->background_color[k];
    }
    sp->two_sided = (opts->flags & OW_SOLID_TWO_SIDED) ? 1 : 0;
    sp->mp.near = opts->near > 0.0f ? opts->near : ow::kMeshDefaultNear;
    sp->mp.cull_back = sp->two_sided ? 0 : 1;
    sp->mp.camera_ok = 1;
    return OW_OK;
}

// the argument checks every form of the draw shares: ow_billboard_draw's, in its order, then the context and the shape
ow_status check_solid_draw(const ow_context *c, const ow_solid *solid, const ow_camera *camera, const ow_solid_options *opts, const void *pixels,
                           const void *rgba, ow::CameraParams *cp, ow::SolidParams *sp) {
    if (!rgba && !pixels) return fail(OW_ERR_INVALID, "null argument: both outputs");
    if (ow_status st = resolve_camera(camera, cp); st != OW_OK) return st;
    if (ow_status st = resolve_solid_options(opts, sp); st != OW_OK) return st;
    if (ow_status st = check_handle(c, solid, "solid"); st != OW_OK) return st;
    sp->mp.camera_ok = ow::mesh_camera_ok(*cp) ? 1 : 0;
    return OW_OK;
}
}  // namespace

namespace ow::readside {
// the number of instances of one draw against the shape
ow_status check_solid_count(const ow_solid *solid, int64_t count) {
    if (count < 0 || count > OW_SOLID_MAX_INSTANCES) return fail(OW_ERR_INVALID, "%lld instances outside [0,%d]", (long long)count, OW_SOLID_MAX_INSTANCES);
    if (count * solid->shape.num_triangles > ow::kSolidMaxProduct || count * solid->shape.num_vertices > ow::kSolidMaxProduct)
        return fail(OW_ERR_INVALID, "%lld instances of %d triangles and %d vertices: more than 2^24 per draw", (long long)count, solid->shape.num_triangles,
                    solid->shape.num_vertices);
    return OW_OK;
}
ow_status check_solid_bodies(const ow_context *c, const ow_solid *solid, const ow_bodies *set, int32_t first, int32_t count) {
    if (ow_status st = check_handle(c, set, "body set"); st != OW_OK) return st;
    if (first < 0 || count < 0 || (int64_t)first + count > set->A.num_bodies)
        return fail(OW_ERR_INVALID, "bodies [%d, %d + %d) outside [0, %d)", first, first, count, set->A.num_bodies);
    return check_solid_count(solid, count);
}

// Where the instances of a draw or a shadow cast come from: a body set's resident pose records and fault flags, or `upload` (host
// transforms: instance_upload_bytes of the caller's scratch at `staging`, copied there on `s` first).
size_t instance_upload_bytes(const float *upload, int count) { return upload ? (size_t)count * ow::kSolidTransformFloats * sizeof(float) : 0; }
ow_status instance_source(const ow_bodies *set, int first, const float *upload, int count, void *staging, hipStream_t s, ow::SolidInstances *in) {
    if (set) *in = ow::SolidInstances{(const float *)(set->A.records + first), set->A.flags + first, (int)(sizeof(ow::BuoyancyBody) / sizeof(float)), count};
    else *in = ow::SolidInstances{(const float *)staging, nullptr, ow::kSolidTransformFloats, count};
    if (!set && count > 0) OW_HIP(hipMemcpyAsync(staging, upload, instance_upload_bytes(upload, count), hipMemcpyHostToDevice, s));
    return OW_OK;
}
}  // namespace ow::readside

namespace {
// The scratch of a draw and its launches on the context's stream, its instances from instance_source.  A block that has to grow while
// launches already enqueued may still read it is replaced behind one synchronisation (sync_before_growth).
ow_status solid_enqueue(ow_context *c, const ow_solid *solid, const ow::CameraParams &cp, const ow::SolidParams &sp, const ow_bodies *set, int first,
                        const float *upload, int count, ow::RenderPixel *pixels_dev, uint32_t *rgba_dev) {
    Layout L;
    L.take(kCounterHead);  // the counters, at 0
    const size_t v_off = L.take((size_t)count * solid->shape.num_vertices * sizeof(ow::MeshVertex));
    const size_t w_off = L.take((size_t)cp.width * cp.height * sizeof(uint64_t));
    const size_t t_off = L.take(instance_upload_bytes(upload, count));
    if (ow_status st = sync_before_growth(c, c->solid, L.total); st != OW_OK) return st;
    if (ow_status st = c->solid.ensure(L.total, 0, 1, "bytes of solid scratch"); st != OW_OK) return st;
    char *base = (char *)c->solid.ptr;
    hipStream_t s = main_stream(c);
    const ow::SolidArrays A{solid->shape, (uint32_t *)base, (ow::MeshVertex *)(base + v_off), (uint64_t *)(base + w_off)};
    ow::SolidInstances in;
    if (ow_status st = instance_source(set, first, upload, count, base + t_off, s, &in); st != OW_OK) return st;
    OW_HIP(ow::launch_solid_draw(A, in, cp, sp, rgba_dev, pixels_dev, s));
    ++c->solid_draws;
    return OW_OK;
}

// a draw in either form (pixel_pass) over the caller's records
ow_status solid_draw(ow_context *c, bool async, const ow_solid *solid, const ow::CameraParams &cp, const ow::SolidParams &sp, const ow_bodies *set, int first,
                     const float *upload, int count, ow_render_pixel *pixels, void *rgba8) {
    return pixel_pass(c, async, (size_t)cp.width * cp.height, rgba8, pixels, [&](uint32_t *rgba_dev, ow::RenderPixel *pixels_dev) {
        return solid_enqueue(c, solid, cp, sp, set, first, upload, count, pixels_dev, rgba_dev);
    });
}
}  // namespace

extern "C" {

void ow_solid_options_default(ow_solid_options *out) {
    if (out) solid_defaults(out);
}

ow_status ow_solid_create(ow_context *c, const float *vertices_xyz, int32_t num_vertices, const int32_t *indices, int32_t num_triangles, ow_solid **out) {
    if (!out) return fail(OW_ERR_INVALID, "null argument");
    *out = nullptr;
    if (num_vertices < 1 || num_triangles < 1 || num_triangles > OW_SOLID_MAX_TRIANGLES || (int64_t)num_vertices > ow::kSolidMaxProduct)
        return fail(OW_ERR_INVALID, "num_vertices must be in [1,2^24] and num_triangles in [1,%d]", OW_SOLID_MAX_TRIANGLES);
    if (!vertices_xyz || !indices) return fail(OW_ERR_INVALID, "null argument");
    for (size_t i = 0; i < (size_t)num_triangles * 3; ++i)
        if (indices[i] < 0 || indices[i] >= num_vertices)
            return fail(OW_ERR_INVALID, "triangle %zu: index %d outside [0,%d)", i / 3, indices[i], num_vertices);
    if (!c) return fail(OW_ERR_INVALID, "null context");
    const size_t nv = (size_t)num_vertices, nt = (size_t)num_triangles;
    Layout L;
    const size_t l_off = L.take(nv * 3 * sizeof(float)), i_off = L.take(nt * 3 * sizeof(int32_t)), b_off = L.take(sizeof(ow::SolidCastBound));
    ow_solid *m;
    if (ow_status st = new_handle(c, L.total, "solid", &m); st != OW_OK) return st;
    char *base = (char *)m->block;
    m->shape = ow::SolidShape{(const float *)(base + l_off), (const int32_t *)(base + i_off), num_vertices, num_triangles};
    m->bound = (ow::SolidCastBound *)(base + b_off);  // written by the shape's first ray cast
    hipStream_t s = main_stream(c);
    const bool enqueued = hipMemcpyAsync((void *)m->shape.local, vertices_xyz, nv * 3 * sizeof(float), hipMemcpyHostToDevice, s) == hipSuccess &&
                          hipMemcpyAsync((void *)m->shape.indices, indices, nt * 3 * sizeof(int32_t), hipMemcpyHostToDevice, s) == hipSuccess;
    return finish_create(c, m, s, enqueued, "solid upload", out);
}

void ow_solid_destroy(ow_context *, ow_solid *solid) {
    if (solid) release_handle(solid);
    delete solid;
}

ow_status ow_solid_draw(ow_context *c, ow_solid *solid, ow_bodies *bodies, int32_t first_body, int32_t body_count, const ow_camera *camera,
                        const ow_solid_options *opts, ow_render_pixel *pixels_inout, void *rgba8_out) {
    ow::CameraParams cp;
    ow::SolidParams sp;
    if (ow_status st = check_solid_draw(c, solid, camera, opts, pixels_inout, rgba8_out, &cp, &sp); st != OW_OK) return st;
    if (ow_status st = check_solid_bodies(c, solid, bodies, first_body, body_count); st != OW_OK) return st;
    return solid_draw(c, false, solid, cp, sp, bodies, first_body, nullptr, body_count, pixels_inout, rgba8_out);
}

ow_status ow_solid_draw_async(ow_context *c, ow_solid *solid, ow_bodies *bodies, int32_t first_body, int32_t body_count, const ow_camera *camera,
                              const ow_solid_options *opts, ow_render_pixel *pixels_dev, void *rgba8_dev) {
    ow::CameraParams cp;
    ow::SolidParams sp;
    if (ow_status st = check_solid_draw(c, solid, camera, opts, pixels_dev, rgba8_dev, &cp, &sp); st != OW_OK) return st;
    if (ow_status st = check_solid_bodies(c, solid, bodies, first_body, body_count); st != OW_OK) return st;
    return solid_draw(c, true, solid, cp, sp, bodies, first_body, nullptr, body_count, pixels_dev, rgba8_dev);
}

ow_status ow_solid_draw_instances(ow_context *c, ow_solid *solid, const float *transforms, int32_t count, const ow_camera *camera,
                                  const ow_solid_options *opts, ow_render_pixel *pixels_inout, void *rgba8_out) {
    if (count < 0 || count > OW_SOLID_MAX_INSTANCES) return fail(OW_ERR_INVALID, "count %d outside [0,%d]", count, OW_SOLID_MAX_INSTANCES);
    if (count > 0 && !transforms) return fail(OW_ERR_INVALID, "null argument");
    ow::CameraParams cp;
    ow::SolidParams sp;
    if (ow_status st = check_solid_draw(c, solid, camera, opts, pixels_inout, rgba8_out, &cp, &sp); st != OW_OK) return st;
    if (ow_status st = check_solid_count(solid, count); st != OW_OK) return st;
    return solid_draw(c, false, solid, cp, sp, nullptr, 0, transforms, count, pixels_inout, rgba8_out);
}

ow_status ow_solid_draw_stats(ow_context *c, uint64_t *draws, uint64_t *skipped_instances, uint64_t *culled, uint64_t *drawn, uint64_t *scratch_bytes) {
    if (!c) return fail(OW_ERR_INVALID, "null context");
    uint64_t n[4];  // no draw yet, no scratch: zeros, and the device is not touched
    if (ow_status st = read_class_counts(c, c->solid.ptr, skipped_instances || culled || drawn, n); st != OW_OK) return st;
    if (skipped_instances) *skipped_instances = n[ow::kSolidSkippedInstances];
    if (culled) *culled = n[ow::kSolidCulled];
    if (drawn) *drawn = n[ow::kSolidLane] + n[ow::kSolidWave];
    if (draws) *draws = c->solid_draws;
    if (scratch_bytes) *scratch_bytes = c->solid.bytes;
    return OW_OK;
}

}  // extern "C"

/* ---- ray casts against the solids (ow_solid_cast.h, ow_solid_cast.hip) ---- */

namespace {
// ow_solid_cast_options (NULL = zeros) -> the cast's constants
ow_status resolve_solid_cast_options(const ow_solid_cast_options *opts, ow::SolidCastParams *cp) {
    static_assert(sizeof(ow_solid_cast_options) == sizeof(ow::SolidCastOptions) && offsetof(ow_solid_cast_options, cull) == offsetof(ow::SolidCastOptions, cull) &&
                      offsetof(ow_solid_cast_options, reserved) == offsetof(ow::SolidCastOptions, reserved) && sizeof(ow_solid_hit) == sizeof(ow::SolidHit) &&
                      offsetof(ow_solid_hit, normal) == offsetof(ow::SolidHit, normal) && offsetof(ow_solid_hit, status) == offsetof(ow::SolidHit, status) &&
                      offsetof(ow_solid_hit, instance) == offsetof(ow::SolidHit, instance) && offsetof(ow_solid_hit, barycentric) == offsetof(ow::SolidHit, barycentric) &&
                      offsetof(ow_solid_hit, reserved) == offsetof(ow::SolidHit, reserved) && OW_SOLID_CAST_TWO_SIDED == ow::kSolidCastTwoSided &&
                      sizeof(ow_raycast_hit) == sizeof(ow::RaycastHit) && offsetof(ow_raycast_hit, status) == offsetof(ow::RaycastHit, status),
                  "record layout");
    cp->two_sided = 0;
    cp->cull = 1;
    if (!opts) return OW_OK;
    if (opts->flags & ~OW_SOLID_CAST_TWO_SIDED) return fail(OW_ERR_INVALID, "unknown solid cast flags 0x%x", opts->flags);
    if (opts->cull != 0 && opts->cull != -1) return fail(OW_ERR_INVALID, "cull %d is neither 0 nor -1", opts->cull);
    if (ow_status st = check_reserved(opts->reserved, "ow_solid_cast_options"); st != OW_OK) return st;
    cp->two_sided = (opts->flags & OW_SOLID_CAST_TWO_SIDED) ? 1 : 0;
    cp->cull = opts->cull == 0 ? 1 : 0;
    return OW_OK;
}

// the argument checks every form of the cast shares: ow_solid_draw's, in its order -- outputs, options, then the context and the shape
ow_status check_solid_cast(const ow_context *c, const ow_solid *solid, const void *rays, int32_t count, const ow_solid_cast_options *opts, const void *out,
                           ow::SolidCastParams *cp) {
    if (count < 0) return fail(OW_ERR_INVALID, "count %d is negative", count);
    if (count > 0 && (!rays || !out)) return fail(OW_ERR_INVALID, "null argument");
    if (ow_status st = resolve_solid_cast_options(opts, cp); st != OW_OK) return st;
    return check_handle(c, solid, "solid");
}

// One cast's scratch and launches on the context's stream, its instances from instance_source.  With host rays the rays, the water records
// and the hit records lie in the scratch as well: the rays (and the records) go up first, the hits come back behind the launches.
ow_status solid_cast_enqueue(ow_context *c, ow_solid *solid, const ow::SolidCastParams &cp, const ow_bodies *set, int first, const float *upload, int instances,
                             const ow_ray *rays, int count, const ow_raycast_hit *water, ow_solid_hit *out, bool host_rays) {
    OW_HIP(hipSetDevice(c->device));
    Layout L;
    L.take(ow::kSolidCastCounterBytes);  // the counters, at 0
    const size_t b_off = L.take((size_t)instances * sizeof(ow::SolidCastBound));
    const size_t t_off = L.take(instance_upload_bytes(upload, instances));
    const size_t r_off = L.take(host_rays ? (size_t)count * sizeof(ow::Ray) : 0);
    const size_t w_off = L.take(host_rays && water ? (size_t)count * sizeof(ow::RaycastHit) : 0);
    const size_t h_off = L.take(host_rays ? (size_t)count * sizeof(ow::SolidHit) : 0);
    if (ow_status st = sync_before_growth(c, c->solid_cast, L.total); st != OW_OK) return st;
    if (ow_status st = c->solid_cast.ensure(L.total, 0, 1, "bytes of solid cast scratch"); st != OW_OK) return st;
    char *base = (char *)c->solid_cast.ptr;
    hipStream_t s = main_stream(c);
    if (!solid->bound_enqueued) {  // once per shape, in stream order ahead of every cast that reads it
        OW_HIP(ow::launch_solid_cast_shape_bound(solid->shape, solid->bound, s));
        solid->bound_enqueued = true;
    }
    const ow::SolidCastArrays A{solid->shape, solid->bound, base, (ow::SolidCastBound *)(base + b_off)};
    ow::SolidInstances in;
    if (ow_status st = instance_source(set, first, upload, instances, base + t_off, s, &in); st != OW_OK) return st;
    const ow::Ray *rays_dev = (const ow::Ray *)rays;
    const ow::RaycastHit *water_dev = (const ow::RaycastHit *)water;
    ow::SolidHit *out_dev = (ow::SolidHit *)out;
    if (host_rays) {
        OW_HIP(hipMemcpyAsync(base + r_off, rays, (size_t)count * sizeof(ow::Ray), hipMemcpyHostToDevice, s));
        if (water) OW_HIP(hipMemcpyAsync(base + w_off, water, (size_t)count * sizeof(ow::RaycastHit), hipMemcpyHostToDevice, s));
        rays_dev = (const ow::Ray *)(base + r_off);
        water_dev = water ? (const ow::RaycastHit *)(base + w_off) : nullptr;
        out_dev = (ow::SolidHit *)(base + h_off);
    }
    OW_HIP(ow::launch_solid_cast(A, in, cp, rays_dev, water_dev, count, out_dev, s));
    ++c->solid_casts;
    if (host_rays) {
        OW_HIP(hipMemcpyAsync(out, out_dev, (size_t)count * sizeof(ow::SolidHit), hipMemcpyDeviceToHost, s));
        return sync_stream(c, 0);
    }
    return OW_OK;
}
}  // namespace

extern "C" {

ow_status ow_cast_bodies(ow_context *c, ow_solid *solid, ow_bodies *bodies, int32_t first_body, int32_t body_count, const ow_ray *rays, int32_t count,
                            const ow_raycast_hit *water_hits, const ow_solid_cast_options *opts, ow_solid_hit *out) {
    ow::SolidCastParams cp;
    if (ow_status st = check_solid_cast(c, solid, rays, count, opts, out, &cp); st != OW_OK) return st;
    if (ow_status st = check_solid_bodies(c, solid, bodies, first_body, body_count); st != OW_OK) return st;
    if (count == 0) return OW_OK;
    return solid_cast_enqueue(c, solid, cp, bodies, first_body, nullptr, body_count, rays, count, water_hits, out, true);
}

ow_status ow_cast_bodies_async(ow_context *c, ow_solid *solid, ow_bodies *bodies, int32_t first_body, int32_t body_count, const ow_ray *rays_dev,
                                  int32_t count, const ow_raycast_hit *water_hits_dev, const ow_solid_cast_options *opts, ow_solid_hit *out_dev) {
    ow::SolidCastParams cp;
    if (ow_status st = check_solid_cast(c, solid, rays_dev, count, opts, out_dev, &cp); st != OW_OK) return st;
    if (ow_status st = check_solid_bodies(c, solid, bodies, first_body, body_count); st != OW_OK) return st;
    if (((uintptr_t)out_dev & 15u) || ((uintptr_t)rays_dev & 3u) || ((uintptr_t)water_hits_dev & 3u))
        return fail(OW_ERR_INVALID, "out_dev must be 16-byte, rays_dev and water_hits_dev 4-byte aligned");
    if (count == 0) return OW_OK;
    return solid_cast_enqueue(c, solid, cp, bodies, first_body, nullptr, body_count, rays_dev, count, water_hits_dev, out_dev, false);
}

ow_status ow_cast_instances(ow_context *c, ow_solid *solid, const float *transforms, int32_t instance_count, const ow_ray *rays, int32_t count,
                                      const ow_raycast_hit *water_hits, const ow_solid_cast_options *opts, ow_solid_hit *out) {
    if (instance_count < 0 || instance_count > OW_SOLID_MAX_INSTANCES)
        return fail(OW_ERR_INVALID, "instance_count %d outside [0,%d]", instance_count, OW_SOLID_MAX_INSTANCES);
    if (instance_count > 0 && !transforms) return fail(OW_ERR_INVALID, "null argument");
    ow::SolidCastParams cp;
    if (ow_status st = check_solid_cast(c, solid, rays, count, opts, out, &cp); st != OW_OK) return st;
    if (ow_status st = check_solid_count(solid, instance_count); st != OW_OK) return st;
    if (count == 0) return OW_OK;
    return solid_cast_enqueue(c, solid, cp, nullptr, 0, transforms, instance_count, rays, count, water_hits, out, true);
}

ow_status ow_cast_stats(ow_context *c, uint64_t *casts, uint64_t *skipped_instances, uint64_t *sphere_tests_passed, uint64_t *pairs_tested,
                                  uint64_t *scratch_bytes) {
    if (!c) return fail(OW_ERR_INVALID, "null context");
    uint64_t skipped = 0, passed = 0, pairs = 0;  // no cast yet, no scratch: zeros, and the device is not touched
    if (c->solid_cast.ptr && (skipped_instances || sphere_tests_passed || pairs_tested)) {
        alignas(8) unsigned char head[ow::kSolidCastCounterBytes];
        OW_HIP(hipSetDevice(c->device));
        if (ow_status st = read_back(c, head, c->solid_cast.ptr, sizeof(head)); st != OW_OK) return st;
        uint32_t sk;
        std::memcpy(&sk, head, sizeof(sk));
        skipped = sk;
        for (int k = 0; k < ow::kSolidCastSlots; ++k) {
            uint64_t two[2];
            std::memcpy(two, head + ow::kSolidCastSumsOffset + (size_t)k * ow::kSolidCastSlotWords * sizeof(uint64_t), sizeof(two));
            passed += two[0];
            pairs += two[1];
        }
    }
    if (skipped_instances) *skipped_instances = skipped;
    if (sphere_tests_passed) *sphere_tests_passed = passed;
    if (pairs_tested) *pairs_tested = pairs;
    if (casts) *casts = c->solid_casts;
    if (scratch_bytes) *scratch_bytes = c->solid_cast.bytes;
    return OW_OK;
}

}  // extern "C"

/* ---- the sun shadows (ow_shadow.h, ow_shadow.hip) ---- */

namespace {
void shadow_frame_defaults(ow_shadow_frame *o) {
    ow_render_options ro;
    render_defaults(&ro);
    std::memset(o, 0, sizeof(*o));
    for (int k = 0; k < 3; ++k) o->light_direction[k] = ro.light_direction[k];
    o->half_extent = 50.0f;
    o->depth_range = 100.0f;
}
// main.tscn:114-116
void shadow_defaults(ow_shadow_options *o) {
    std::memset(o, 0, sizeof(*o));
    o->bias = 0.0f;
    o->normal_bias = 6.464f;
    o->opacity = 0.8f;
    o->filter_taps = 5;
}

// ow_shadow_frame -> the frame's constants for a map of side `size` (ow_shadow.h shadow_params), after the checks
ow_status resolve_shadow_frame(const ow_shadow_frame *f, int size, ow::ShadowParams *P) {
    static_assert(sizeof(ow_shadow_frame) == sizeof(ow::ShadowFrame) && offsetof(ow_shadow_frame, center) == offsetof(ow::ShadowFrame, center) &&
                      offsetof(ow_shadow_frame, flags) == offsetof(ow::ShadowFrame, flags) &&
                      offsetof(ow_shadow_frame, lane_box) == offsetof(ow::ShadowFrame, lane_box) &&
                      offsetof(ow_shadow_frame, reserved) == offsetof(ow::ShadowFrame, reserved) && sizeof(ow_shadow_options) == sizeof(ow::ShadowOptions) &&
                      offsetof(ow_shadow_options, flags) == offsetof(ow::ShadowOptions, flags) &&
                      offsetof(ow_shadow_options, reserved) == offsetof(ow::ShadowOptions, reserved) && OW_RAY_SHADOWED == ow::kRayShadowed &&
                      OW_RAY_ENVIRONMENT == ow::kRayEnvironmentDone && OW_SHADOW_CAST_BOTH_SIDES == ow::kShadowCastBothSides &&
                      OW_SHADOW_RECEIVE_WATER == ow::kShadowReceiveWater && OW_SHADOW_MIN_SIZE == ow::kShadowMinSize && OW_SHADOW_MAX_SIZE == ow::kShadowMaxSize,
                  "record layout");
    if (!f) return fail(OW_ERR_INVALID, "null frame");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(f->light_direction[k]) || !std::isfinite(f->center[k]))
            return fail(OW_ERR_INVALID, "ow_shadow_frame: light_direction or center is not finite");
    if (!(f->half_extent > 0.0f && f->half_extent <= ow::kShadowRangeMax)) return fail(OW_ERR_INVALID, "ow_shadow_frame: half_extent outside (0,1e6]");
    if (!(f->depth_range > 0.0f && f->depth_range <= ow::kShadowRangeMax)) return fail(OW_ERR_INVALID, "ow_shadow_frame: depth_range outside (0,1e6]");
    if (ow_status st = resolve_lane_box(f->lane_box, nullptr); st != OW_OK) return st;
    if (f->flags & ~OW_SHADOW_CAST_BOTH_SIDES) return fail(OW_ERR_INVALID, "unknown shadow frame flags 0x%x", f->flags);
    if (ow_status st = check_reserved(f->reserved, "ow_shadow_frame"); st != OW_OK) return st;
    ow::ShadowFrame fr;
    std::memcpy(&fr, f, sizeof(fr));
    *P = ow::shadow_params(fr, size);
    if (!P->ok) return fail(OW_ERR_INVALID, "light_direction has zero length");
    return OW_OK;
}

ow_status resolve_shadow_options(const ow_shadow_options *opts, ow::ShadowApply *ap) {
    ow_shadow_options def;
    opts = or_defaults(opts, &def, shadow_defaults);
    if (!in_range(opts->bias, -ow::kShadowRangeMax, ow::kShadowRangeMax)) return fail(OW_ERR_INVALID, "ow_shadow_options: bias outside [-1e6,1e6]");
    if (!in_range(opts->normal_bias, -ow::kShadowRangeMax, ow::kShadowRangeMax)) return fail(OW_ERR_INVALID, "ow_shadow_options: normal_bias outside [-1e6,1e6]");
    if (!in_range(opts->opacity, 0.0f, 1.0f)) return fail(OW_ERR_INVALID, "ow_shadow_options: opacity outside [0,1]");
    const int taps = opts->filter_taps == 0 ? 5 : opts->filter_taps;
    if (taps < 1 || taps > 9 || taps % 2 == 0) return fail(OW_ERR_INVALID, "filter_taps %d is not one of 0, 1, 3, 5, 7, 9", opts->filter_taps);
    if (opts->flags & ~OW_SHADOW_RECEIVE_WATER) return fail(OW_ERR_INVALID, "unknown shadow flags 0x%x", opts->flags);
    if (ow_status st = check_reserved(opts->reserved, "ow_shadow_options"); st != OW_OK) return st;
    ow::ShadowOptions so;
    std::memcpy(&so, opts, sizeof(so));
    *ap = ow::shadow_apply_params(so, true);
    return OW_OK;
}

ow_status check_shadow_map(const ow_context *c, const ow_shadow_map *map) { return check_handle(c, map, "shadow map"); }

// The pass in either form (pixel_pass).  The argument checks both forms share: ow_solid_draw's, in its order, then the context and the map.
ow_status shadow_apply(ow_context *c, bool async, const ow_shadow_map *map, const ow_camera *camera, const ow_shadow_options *opts, ow_render_pixel *pixels,
                       void *rgba8) {
    ow::CameraParams cp;
    ow::ShadowApply ap;
    if (!pixels) return fail(OW_ERR_INVALID, "null argument: the records");
    if (ow_status st = resolve_camera(camera, &cp); st != OW_OK) return st;
    if (ow_status st = resolve_shadow_options(opts, &ap); st != OW_OK) return st;
    if (ow_status st = check_shadow_map(c, map); st != OW_OK) return st;
    ap.camera_ok = ow::mesh_camera_ok(cp) ? 1 : 0;
    return pixel_pass(c, async, (size_t)cp.width * cp.height, rgba8, pixels, [&](uint32_t *rgba_dev, ow::RenderPixel *pixels_dev) {
        OW_HIP(ow::launch_shadow_apply(map->map, cp, map->P, ap, pixels_dev, rgba_dev, main_stream(c)));
        return OW_OK;
    });
}

// One cast's launches on the context's stream, its instances from instance_source (an upload is copied into the map's scratch first).
ow_status shadow_cast_enqueue(ow_context *c, ow_shadow_map *map, const ow_solid *solid, const ow_bodies *set, int first, const float *upload, int count) {
    if (!map->P.ok) return fail(OW_ERR_STATE, "the shadow map has no frame: ow_shadow_map_begin first");
    OW_HIP(hipSetDevice(c->device));
    Layout L;
    const size_t v_off = L.take((size_t)count * solid->shape.num_vertices * sizeof(ow::ShadowVertex));
    const size_t t_off = L.take(instance_upload_bytes(upload, count));
    if (ow_status st = sync_before_growth(c, map->scratch, L.total); st != OW_OK) return st;
    if (ow_status st = map->scratch.ensure(L.total, 0, 1, "bytes of shadow scratch"); st != OW_OK) return st;
    char *base = (char *)map->scratch.ptr;
    hipStream_t s = main_stream(c);
    const ow::ShadowArrays A{solid->shape, map->counters, (ow::ShadowVertex *)(base + v_off), map->map};
    ow::SolidInstances in;
    if (ow_status st = instance_source(set, first, upload, count, base + t_off, s, &in); st != OW_OK) return st;
    OW_HIP(ow::launch_shadow_cast(A, in, map->P, s));
    ++map->casts;
    map->instances_triangles += (uint64_t)count * solid->shape.num_triangles;
    return OW_OK;
}
}  // namespace

extern "C" {

void ow_shadow_frame_default(ow_shadow_frame *out) {
    if (out) shadow_frame_defaults(out);
}
void ow_shadow_options_default(ow_shadow_options *out) {
    if (out) shadow_defaults(out);
}

ow_status ow_shadow_map_create(ow_context *c, int32_t size, ow_shadow_map **out) {
    if (!out) return fail(OW_ERR_INVALID, "null argument");
    if (size < OW_SHADOW_MIN_SIZE || size > OW_SHADOW_MAX_SIZE) return fail(OW_ERR_INVALID, "shadow map size %d outside [%d,%d]", size, OW_SHADOW_MIN_SIZE, OW_SHADOW_MAX_SIZE);
    if (!c) return fail(OW_ERR_INVALID, "null context");
    Layout L;
    const size_t c_off = L.take(kCounterHead), m_off = L.take((size_t)size * size * sizeof(uint32_t));
    ow_shadow_map *map;
    if (ow_status st = new_handle(c, L.total, "shadow map", &map); st != OW_OK) return st;
    char *base = (char *)map->block;
    map->size = size;
    map->device = c->device;
    map->counters = (uint32_t *)(base + c_off);
    map->map = (uint32_t *)(base + m_off);
    hipStream_t s = main_stream(c);
    const bool enqueued = ow::launch_shadow_clear(ow::ShadowArrays{{}, map->counters, nullptr, map->map}, size, s) == hipSuccess;
    return finish_create(c, map, s, enqueued, "shadow map clear", out);
}

void ow_shadow_map_destroy(ow_context *, ow_shadow_map *map) {
    if (!map) return;
    release_handle(map);
    (void)hipSetDevice(map->device);  // an orphan's scratch is still there: ow_destroy frees the blocks
    map->scratch.release();
    delete map;
}

ow_status ow_shadow_map_begin(ow_context *c, ow_shadow_map *map, const ow_shadow_frame *frame) {
    ow::ShadowParams P;
    if (ow_status st = resolve_shadow_frame(frame, OW_SHADOW_MIN_SIZE, &P); st != OW_OK) return st;  // the checks, before the map is looked at
    if (ow_status st = check_shadow_map(c, map); st != OW_OK) return st;
    if (ow_status st = resolve_shadow_frame(frame, map->size, &P); st != OW_OK) return st;
    OW_HIP(hipSetDevice(c->device));
    OW_HIP(ow::launch_shadow_clear(ow::ShadowArrays{{}, map->counters, nullptr, map->map}, map->size, main_stream(c)));
    map->P = P;
    map->casts = map->instances_triangles = 0;
    return OW_OK;
}

ow_status ow_shadow_map_cast(ow_context *c, ow_shadow_map *map, ow_solid *solid, ow_bodies *bodies, int32_t first_body, int32_t body_count) {
    if (ow_status st = check_shadow_map(c, map); st != OW_OK) return st;
    if (ow_status st = check_handle(c, solid, "solid"); st != OW_OK) return st;
    if (ow_status st = check_solid_bodies(c, solid, bodies, first_body, body_count); st != OW_OK) return st;
    return shadow_cast_enqueue(c, map, solid, bodies, first_body, nullptr, body_count);
}

ow_status ow_shadow_map_cast_instances(ow_context *c, ow_shadow_map *map, ow_solid *solid, const float *transforms, int32_t count) {
    if (count < 0 || count > OW_SOLID_MAX_INSTANCES) return fail(OW_ERR_INVALID, "count %d outside [0,%d]", count, OW_SOLID_MAX_INSTANCES);
    if (count > 0 && !transforms) return fail(OW_ERR_INVALID, "null argument");
    if (ow_status st = check_shadow_map(c, map); st != OW_OK) return st;
    if (ow_status st = check_handle(c, solid, "solid"); st != OW_OK) return st;
    if (ow_status st = check_solid_count(solid, count); st != OW_OK) return st;
    if (ow_status st = shadow_cast_enqueue(c, map, solid, nullptr, 0, transforms, count); st != OW_OK) return st;
    return sync_stream(c, 0);
}

ow_status ow_shadow_map_read(ow_context *c, ow_shadow_map *map, float *depth_out) {
    if (!depth_out) return fail(OW_ERR_INVALID, "null argument");
    if (ow_status st = check_shadow_map(c, map); st != OW_OK) return st;
    return read_back(c, depth_out, map->map, (size_t)map->size * map->size * sizeof(float));
}

ow_status ow_shadow_apply(ow_context *c, ow_shadow_map *map, const ow_camera *camera, const ow_shadow_options *opts, ow_render_pixel *pixels_inout,
                          void *rgba8_out) {
    return shadow_apply(c, false, map, camera, opts, pixels_inout, rgba8_out);
}

ow_status ow_shadow_apply_async(ow_context *c, ow_shadow_map *map, const ow_camera *camera, const ow_shadow_options *opts, ow_render_pixel *pixels_dev,
                                void *rgba8_dev) {
    return shadow_apply(c, true, map, camera, opts, pixels_dev, rgba8_dev);
}

ow_status ow_shadow_stats(ow_context *c, ow_shadow_map *map, uint64_t *casts, uint64_t *skipped_instances, uint64_t *culled, uint64_t *drawn,
                          uint64_t *scratch_bytes) {
    if (ow_status st = check_shadow_map(c, map); st != OW_OK) return st;
    uint64_t n[4];
    if (ow_status st = read_class_counts(c, map->counters, skipped_instances || culled || drawn, n); st != OW_OK) return st;
    if (skipped_instances) *skipped_instances = n[ow::kShadowSkippedInstances];
    if (culled) *culled = n[ow::kShadowCulled];
    if (drawn) *drawn = n[ow::kShadowLane] + n[ow::kShadowWave];
    if (casts) *casts = map->casts;
    if (scratch_bytes) *scratch_bytes = map->scratch.bytes;
    return OW_OK;
}

}  // extern "C"

// ow_points_host.hip -- the calls that read the maps at points, along rays and through a camera: ow_sample_surface, ow_query_*, the velocity
// layers (ow_update_velocity .. ow_query_velocity), ow_raycast_surface and ow_render_view, over the kernels of ow_consumer.hip and
// ow_velocity.hip.  The point and ray round trips also serve a group's gathered arrays (ow_internal.h, ow_group.hip).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "ow_consumer_host.h"

using namespace ow::readside;
using ow::check_cascade, ow::fail, ow::layer_mask, ow::main_stream, ow::plane, ow::refuse_faulted, ow::sync_stream;

namespace ow {
ow_status points_round_trip(const MapsView &v, DeviceScratch &scratch, const float *xz, int count, const float *map_scales, int num_cascades,
                            const QueryParams *qp, const u16x4 *vel, void *out) {
    static_assert(sizeof(SurfaceQuery) >= sizeof(SurfaceSample) && sizeof(SurfaceQuery) >= sizeof(SurfaceVelocity), "the record block holds any kind");
    constexpr size_t kPoint = sizeof(SurfaceQuery) + 2 * sizeof(float);  // the records first, the points behind them
    if (ow_status st = scratch.ensure((size_t)count * kPoint, 4096 * kPoint, kPoint, "query points"); st != OW_OK) return st;
    float *xz_dev = (float *)((char *)scratch.ptr + (size_t)count * sizeof(SurfaceQuery));
    const SurfaceScales sc = surface_scales(map_scales, num_cascades);
    OW_HIP(hipMemcpyAsync(xz_dev, xz, (size_t)count * 2 * sizeof(float), hipMemcpyHostToDevice, v.stream));
    if (!qp) OW_HIP(launch_sample_surface(v.n, num_cascades, v.buf, xz_dev, count, sc, (SurfaceSample *)scratch.ptr, v.stream));
    else if (vel) OW_HIP(launch_query_velocity(v.n, num_cascades, v.buf, vel, xz_dev, count, sc, *qp, (SurfaceVelocity *)scratch.ptr, v.stream));
    else OW_HIP(launch_query_surface(v.n, num_cascades, v.buf, xz_dev, count, sc, *qp, (SurfaceQuery *)scratch.ptr, v.stream));
    const size_t record = !qp ? sizeof(SurfaceSample) : vel ? sizeof(SurfaceVelocity) : sizeof(SurfaceQuery);
    OW_HIP(hipMemcpyAsync(out, scratch.ptr, (size_t)count * record, hipMemcpyDeviceToHost, v.stream));
    return OW_OK;
}

ow_status resolve_query_options(const ow_query_options *o, QueryParams *qp) {
    qp->max_iterations = kQueryDefaultIterations;
    qp->tolerance = kQueryDefaultTolerance;
    qp->falloff = 0;
    qp->center[0] = qp->center[1] = 0.0f;
    if (!o) return OW_OK;
    if (o->max_iterations < 0 || o->max_iterations > kQueryMaxIterations)
        return fail(OW_ERR_INVALID, "max_iterations %d outside [0,%d]", o->max_iterations, kQueryMaxIterations);
    if (o->flags & ~OW_QUERY_DISTANCE_FALLOFF) return fail(OW_ERR_INVALID, "unknown query flags 0x%x", o->flags);
    if (!std::isfinite(o->tolerance)) return fail(OW_ERR_INVALID, "tolerance is not finite");
    if (o->max_iterations > 0) qp->max_iterations = o->max_iterations;
    if (o->tolerance > 0.0f) qp->tolerance = o->tolerance;
    if (o->flags & OW_QUERY_DISTANCE_FALLOFF) {
        if (!std::isfinite(o->falloff_center_xz[0]) || !std::isfinite(o->falloff_center_xz[1]))
            return fail(OW_ERR_INVALID, "falloff_center_xz is not finite");
        qp->falloff = 1;
        qp->center[0] = o->falloff_center_xz[0];
        qp->center[1] = o->falloff_center_xz[1];
    }
    return OW_OK;
}
}  // namespace ow

namespace {
// a synchronous point call on the context's own maps, its arguments checked; velocity: behind a refresh of the layers it reads
ow_status context_points(ow_context *c, const float *xz, int count, const float *map_scales, int num_cascades, const ow::QueryParams *qp, bool velocity,
                         void *out) {
    OW_HIP(hipSetDevice(c->device));
    if (velocity)
        if (ow_status st = velocity_refresh(c, layer_mask(num_cascades)); st != OW_OK) return st;
    if (ow_status st = ow::points_round_trip(view_of(c), c->query_scratch, xz, count, map_scales, num_cascades, qp, velocity ? c->vel : nullptr, out);
        st != OW_OK)
        return st;
    return sync_stream(c, layer_mask(num_cascades));
}

// ---- the velocity layers (ow_velocity_kernels.h), down to ow_velocity_stats ------------------------------------------------------------
// V, its intermediate and its twiddle table, on first use (on the context's device; V starts zeroed, in stream order)
ow_status velocity_buffers(ow_context *c) {
    if (c->vel) return OW_OK;
    const size_t pl = plane(c);
    const int slots = std::min(ow::vel_batch(c->n), c->cascades);
    if (hipMalloc((void **)&c->vel_tw, (size_t)c->n * sizeof(ow::cplx)) != hipSuccess ||
        hipMalloc((void **)&c->vel_scratch, (size_t)slots * ow::vel_scratch_bytes(c->n)) != hipSuccess ||
        hipMalloc((void **)&c->vel, (size_t)c->cascades * pl * sizeof(ow::u16x4)) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(c->vel_tw);
        (void)hipFree(c->vel_scratch);
        (void)hipFree(c->vel);
        c->vel_tw = c->vel_scratch = nullptr;
        c->vel = nullptr;
        return fail(OW_ERR_NOMEM, "hipMalloc failed for the velocity layers (%d x %d^2) and their intermediate", c->cascades, c->n);
    }
    c->vel_slots = slots;
    OW_HIP(ow::launch_velocity_twiddles(c->n, c->vel_tw, main_stream(c)));
    OW_HIP(hipMemsetAsync(c->vel, 0, (size_t)c->cascades * pl * sizeof(ow::u16x4), main_stream(c)));
    return OW_OK;
}
}  // namespace

namespace ow::readside {
// The layers of `mask` (inside [0, cascades)) whose velocity is stale are recomputed, in stream order behind everything the context has
// enqueued, from the resident spectrum and the words their current maps were made with (pc_words[i].modulate); the others are skipped.
// A layer never computed is OW_ERR_STATE, a faulted one is refused as its maps are, and so is one whose spectrum is newer than its maps.
ow_status velocity_refresh(ow_context *c, uint32_t mask) {
    for (int i = 0; i < c->cascades; ++i)
        if ((mask >> i & 1u) && !c->pc_valid[i]) return fail(OW_ERR_STATE, "cascade %d has not been computed yet: it has no velocity", i);
    if (ow_status st = refuse_faulted(c, mask); st != OW_OK) return st;
    if (c->spectrum_ahead & mask)
        return fail(OW_ERR_STATE, "layer mask 0x%x: the resident spectrum is newer than the maps (a failed batch regenerated it): recompute the layers first",
                    c->spectrum_ahead & mask);
    if (ow_status st = velocity_buffers(c); st != OW_OK) return st;
    const uint32_t todo = mask & c->velocity_stale;
    c->vel_skipped += (uint64_t)__builtin_popcount(mask & ~todo);
    ow::VelocityArgs args;
    std::memset(&args, 0, sizeof(args));
    auto word = [](uint32_t w) {
        float f;
        std::memcpy(&f, &w, 4);
        return f;
    };
    auto flush = [&]() -> ow_status {
        if (args.count == 0) return OW_OK;
        OW_HIP(ow::launch_velocity(c->n, args, c->buf, c->vel_tw, c->vel_scratch, c->vel, main_stream(c)));
        for (int k = 0; k < args.count; ++k) c->velocity_stale &= ~(1u << args.cascade[k]);
        c->vel_computed += (uint64_t)args.count;
        args.count = 0;
        return OW_OK;
    };
    for (int i = 0; i < c->cascades; ++i) {
        if (!(todo >> i & 1u)) continue;
        const uint32_t *m = c->pc_words[i].modulate;
        args.cascade[args.count] = i;
        args.tile_x[args.count] = word(m[0]);
        args.tile_y[args.count] = word(m[1]);
        args.time[args.count] = word(m[3]);
        if (++args.count == c->vel_slots)
            if (ow_status st = flush(); st != OW_OK) return st;
    }
    return flush();
}
}  // namespace ow::readside

namespace {
ow_status check_velocity_mask(const ow_context *c, uint32_t mask) {
    if (!c) return fail(OW_ERR_INVALID, "null context");
    if (mask & ~layer_mask(c->cascades)) return fail(OW_ERR_INVALID, "cascade_mask 0x%x names layers outside [0,%d)", mask, c->cascades);
    return OW_OK;
}
// every layer that has been computed
uint32_t computed_layers(const ow_context *c) {
    uint32_t m = 0;
    for (int i = 0; i < c->cascades; ++i)
        if (c->pc_valid[i]) m |= 1u << i;
    return m;
}
}  // namespace

extern "C" {

ow_status ow_update_velocity(ow_context *c, uint32_t cascade_mask) {
    if (ow_status st = check_velocity_mask(c, cascade_mask); st != OW_OK) return st;
    if (cascade_mask == 0) return OW_OK;
    OW_HIP(hipSetDevice(c->device));
    return velocity_refresh(c, cascade_mask);
}

ow_status ow_get_velocity_ptrs(ow_context *c, void **velocity_map, size_t *layer_stride_bytes) {
    if (!c) return fail(OW_ERR_INVALID, "null context");
    if (!velocity_map && !layer_stride_bytes) return fail(OW_ERR_INVALID, "null output");
    OW_HIP(hipSetDevice(c->device));
    if (ow_status st = velocity_buffers(c); st != OW_OK) return st;
    if (ow_status st = velocity_refresh(c, computed_layers(c)); st != OW_OK) return st;
    if (velocity_map) *velocity_map = c->vel;
    if (layer_stride_bytes) *layer_stride_bytes = plane(c) * sizeof(ow::u16x4);
    return OW_OK;
}

ow_status ow_get_velocity_map(ow_context *c, int32_t cascade, void *velocity_rgba16f) {
    if (ow_status st = check_cascade(c, cascade); st != OW_OK) return st;
    if (!velocity_rgba16f) return fail(OW_ERR_INVALID, "null output");
    OW_HIP(hipSetDevice(c->device));
    if (ow_status st = velocity_refresh(c, 1u << cascade); st != OW_OK) return st;
    OW_HIP(hipMemcpyAsync(velocity_rgba16f, c->vel + cascade * plane(c), plane(c) * sizeof(ow::u16x4), hipMemcpyDeviceToHost, main_stream(c)));
    return sync_stream(c, 1u << cascade);
}

ow_status ow_velocity_stats(const ow_context *c, uint64_t *layers_computed, uint64_t *layers_skipped) {
    if (!c) return fail(OW_ERR_INVALID, "null context");
    if (layers_computed) *layers_computed = c->vel_computed;
    if (layers_skipped) *layers_skipped = c->vel_skipped;
    return OW_OK;
}

/* ---- samples and queries at points (ow_surface.h) ---- */

ow_status ow_sample_surface(ow_context *c, const float *xz, int32_t count, const float *map_scales, int32_t num_cascades,
                            ow_surface_sample *out) {
    static_assert(sizeof(ow_surface_sample) == sizeof(ow::SurfaceSample) && sizeof(ow_surface_sample) == 64, "record layout");
    if (ow_status st = check_point_query(c, count, num_cascades); st != OW_OK) return st;
    if (count == 0) return OW_OK;
    if (!xz || !map_scales || !out) return fail(OW_ERR_INVALID, "null argument");
    return context_points(c, xz, count, map_scales, num_cascades, nullptr, false, out);
}

ow_status ow_query_surface(ow_context *c, const float *xz, int32_t count, const float *map_scales, int32_t num_cascades,
                           const ow_query_options *opts, ow_surface_query *out) {
    static_assert(sizeof(ow_surface_query) == sizeof(ow::SurfaceQuery) && offsetof(ow_surface_query, sample) == offsetof(ow::SurfaceQuery, sample) &&
                      offsetof(ow_surface_query, world_xz) == offsetof(ow::SurfaceQuery, world_xz),
                  "record layout");
    ow::QueryParams qp;
    if (ow_status st = check_point_call(c, xz, count, map_scales, num_cascades, opts, ow::resolve_query_options, &qp, out); st != OW_OK) return st;
    if (count == 0) return OW_OK;
    return context_points(c, xz, count, map_scales, num_cascades, &qp, false, out);
}

ow_status ow_query_surface_async(ow_context *c, const float *xz_dev, int32_t count, const float *map_scales, int32_t num_cascades,
                                 const ow_query_options *opts, ow_surface_query *out_dev) {
    ow::QueryParams qp;
    if (ow_status st = check_point_call(c, xz_dev, count, map_scales, num_cascades, opts, ow::resolve_query_options, &qp, out_dev); st != OW_OK) return st;
    if (count == 0) return OW_OK;
    if (ow_status st = begin_async(c, num_cascades); st != OW_OK) return st;
    const ow::MapsView v = view_of(c);
    OW_HIP(ow::launch_query_surface(v.n, num_cascades, v.buf, xz_dev, count, surface_scales(map_scales, num_cascades), qp, (ow::SurfaceQuery *)out_dev, v.stream));
    return OW_OK;
}

ow_status ow_query_velocity(ow_context *c, const float *xz, int32_t count, const float *map_scales, int32_t num_cascades,
                            const ow_query_options *opts, ow_surface_velocity *out) {
    static_assert(sizeof(ow_surface_velocity) == sizeof(ow::SurfaceVelocity) && offsetof(ow_surface_velocity, converged) == offsetof(ow::SurfaceVelocity, converged),
                  "record layout");
    ow::QueryParams qp;
    if (ow_status st = check_point_call(c, xz, count, map_scales, num_cascades, opts, ow::resolve_query_options, &qp, out); st != OW_OK) return st;
    if (count == 0) return OW_OK;
    return context_points(c, xz, count, map_scales, num_cascades, &qp, true, out);
}

ow_status ow_query_velocity_async(ow_context *c, const float *xz_dev, int32_t count, const float *map_scales, int32_t num_cascades,
                                  const ow_query_options *opts, ow_surface_velocity *out_dev) {
    ow::QueryParams qp;
    if (ow_status st = check_point_call(c, xz_dev, count, map_scales, num_cascades, opts, ow::resolve_query_options, &qp, out_dev); st != OW_OK) return st;
    if (count == 0) return OW_OK;
    if (ow_status st = begin_async(c, num_cascades); st != OW_OK) return st;
    if (ow_status st = velocity_refresh(c, layer_mask(num_cascades)); st != OW_OK) return st;
    const ow::MapsView v = view_of(c);
    OW_HIP(ow::launch_query_velocity(v.n, num_cascades, v.buf, c->vel, xz_dev, count, surface_scales(map_scales, num_cascades), qp, (ow::SurfaceVelocity *)out_dev,
                                     v.stream));
    return OW_OK;
}

}  // extern "C"

/* ---- ray casts (ow_raycast.h; the kernel in ow_consumer.hip) ---- */

namespace ow::readside {
// the per-cascade bound words of the slab on the current device, allocated by the first call that needs them
ow_status ray_bound_words(uint32_t **bound) {
    if (!*bound && hipMalloc((void **)bound, OW_MAX_CASCADES * sizeof(uint32_t)) != hipSuccess) {
        *bound = nullptr;
        return fail(OW_ERR_NOMEM, "hipMalloc failed for the ray-cast bound words");
    }
    return OW_OK;
}
}  // namespace ow::readside

namespace ow {
ow_status resolve_raycast_options(const ow_raycast_options *o, RaycastParams *rp) {
    if (ow_status st = resolve_query_options(o ? &o->query : nullptr, &rp->qp); st != OW_OK) return st;
    rp->water_level = 0.0f;
    rp->spacing = kRayDefaultSpacing;
    rp->tolerance = kRayDefaultTolerance;
    rp->max_samples = kRayDefaultMaxSamples;
    if (!o) return OW_OK;
    if (!std::isfinite(o->water_level) || !std::isfinite(o->sample_spacing) || !std::isfinite(o->tolerance))
        return fail(OW_ERR_INVALID, "water_level, sample_spacing and tolerance must be finite");
    if (o->max_samples < 0 || o->max_samples > kRayMaxSamples)
        return fail(OW_ERR_INVALID, "max_samples %d outside [0,%d]", o->max_samples, kRayMaxSamples);
    if (ow_status st = check_reserved(o->reserved, "ow_raycast_options"); st != OW_OK) return st;
    rp->water_level = o->water_level;
    if (o->sample_spacing > 0.0f) rp->spacing = o->sample_spacing;
    if (o->tolerance > 0.0f) rp->tolerance = o->tolerance;
    if (o->max_samples > 0) rp->max_samples = o->max_samples;
    return OW_OK;
}

ow_status rays_round_trip(const MapsView &v, DeviceScratch &scratch, uint32_t **bound, const ow_ray *rays, int count, const float *map_scales,
                          int num_cascades, const RaycastParams &rp, ow_raycast_hit *out) {
    constexpr size_t kRay = sizeof(RaycastHit) + sizeof(Ray);  // the records first, the rays behind them
    if (ow_status st = ray_bound_words(bound); st != OW_OK) return st;
    if (ow_status st = scratch.ensure((size_t)count * kRay, 1024 * kRay, kRay, "rays"); st != OW_OK) return st;
    Ray *rays_dev = (Ray *)((char *)scratch.ptr + (size_t)count * sizeof(RaycastHit));
    OW_HIP(hipMemcpyAsync(rays_dev, rays, (size_t)count * sizeof(Ray), hipMemcpyHostToDevice, v.stream));
    OW_HIP(launch_raycast(v.n, num_cascades, v.buf, rays_dev, count, surface_scales(map_scales, num_cascades), rp, *bound, (RaycastHit *)scratch.ptr, v.stream));
    OW_HIP(hipMemcpyAsync(out, scratch.ptr, (size_t)count * sizeof(RaycastHit), hipMemcpyDeviceToHost, v.stream));
    return OW_OK;
}
}  // namespace ow

extern "C" {

ow_status ow_raycast_surface(ow_context *c, const ow_ray *rays, int32_t count, const float *map_scales, int32_t num_cascades,
                             const ow_raycast_options *opts, ow_raycast_hit *out) {
    static_assert(sizeof(ow_ray) == sizeof(ow::Ray) && sizeof(ow_raycast_hit) == sizeof(ow::RaycastHit) &&
                      offsetof(ow_raycast_hit, query) == offsetof(ow::RaycastHit, query) &&
                      offsetof(ow_raycast_hit, slab_half_height) == offsetof(ow::RaycastHit, slab_half_height) &&
                      offsetof(ow_ray, direction) == offsetof(ow::Ray, direction),
                  "record layout");
    ow::RaycastParams rp;
    if (ow_status st = check_point_call(c, rays, count, map_scales, num_cascades, opts, ow::resolve_raycast_options, &rp, out); st != OW_OK) return st;
    if (count == 0) return OW_OK;
    OW_HIP(hipSetDevice(c->device));
    if (ow_status st = ow::rays_round_trip(view_of(c), c->ray_scratch, &c->ray_bound, rays, count, map_scales, num_cascades, rp, out); st != OW_OK) return st;
    return sync_stream(c, layer_mask(num_cascades));
}

ow_status ow_raycast_surface_async(ow_context *c, const ow_ray *rays_dev, int32_t count, const float *map_scales, int32_t num_cascades,
                                   const ow_raycast_options *opts, ow_raycast_hit *out_dev) {
    ow::RaycastParams rp;
    if (ow_status st = check_point_call(c, rays_dev, count, map_scales, num_cascades, opts, ow::resolve_raycast_options, &rp, out_dev); st != OW_OK) return st;
    if (count == 0) return OW_OK;
    if (ow_status st = begin_async(c, num_cascades); st != OW_OK) return st;
    if (ow_status st = ray_bound_words(&c->ray_bound); st != OW_OK) return st;
    const ow::MapsView v = view_of(c);
    OW_HIP(ow::launch_raycast(v.n, num_cascades, v.buf, (const ow::Ray *)rays_dev, count, surface_scales(map_scales, num_cascades), rp, c->ray_bound,
                              (ow::RaycastHit *)out_dev, v.stream));
    return OW_OK;
}

}  // extern "C"

/* ---- camera views (ow_render.h; the kernel in ow_consumer.hip) ---- */

namespace ow::readside {
// the reference scene's material and sun (ow_render_options_default)
void render_defaults(ow_render_options *o) {
    std::memset(o, 0, sizeof(*o));
    const float water[3] = {0.0100228256f, 0.019606648f, 0.0272117816f};  // Color(0.1, 0.15, 0.18).srgb_to_linear(), water.gd:14-15
    const float foam[3] = {0.491905034f, 0.406448305f, 0.34239164f};      // Color(0.73, 0.67, 0.62).srgb_to_linear(), water.gd:17-18
    const float sun[3] = {0.321197f, 0.18296f, 0.929171f};                // the basis' +Z column, main.tscn:113
    const float ambient[3] = {0.05f, 0.08f, 0.10f}, sky[3] = {0.25f, 0.40f, 0.60f};
    for (int k = 0; k < 3; ++k) {
        o->water_color[k] = water[k];
        o->foam_color[k] = foam[k];
        o->light_direction[k] = sun[k];
        o->light_color[k] = 1.0f;
        o->ambient_color[k] = ambient[k];
        o->sky_color[k] = sky[k];
    }
    o->roughness = 0.65f;       // mat_water.tres:8
    o->normal_strength = 1.0f;  // mat_water.tres:9
}

// ow_render_options (NULL = the defaults) -> the hit's settings and the shading's; the uniform-only constants in FP64, narrowed once
ow_status resolve_render_options(const ow_render_options *opts, ow::RaycastParams *rp, ow::ShadeParams *sp) {
    ow_render_options def;
    opts = or_defaults(opts, &def, render_defaults);
    if (ow_status st = ow::resolve_raycast_options(&opts->raycast, rp); st != OW_OK) return st;
    const float *vec[6] = {opts->water_color, opts->foam_color, opts->light_direction, opts->light_color, opts->ambient_color, opts->sky_color};
    for (const float *v : vec)
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(v[k])) return fail(OW_ERR_INVALID, "ow_render_options: a colour or the light direction is not finite");
    if (!(opts->roughness >= 0.0f && opts->roughness <= 1.0f)) return fail(OW_ERR_INVALID, "roughness outside [0,1]");
    if (!(opts->normal_strength >= 0.0f && opts->normal_strength <= 1.0f)) return fail(OW_ERR_INVALID, "normal_strength outside [0,1]");
    if (opts->flags != 0u) return fail(OW_ERR_INVALID, "unknown render flags 0x%x", opts->flags);
    if (ow_status st = check_reserved(opts->reserved, "ow_render_options"); st != OW_OK) return st;
    const double lx = opts->light_direction[0], ly = opts->light_direction[1], lz = opts->light_direction[2];
    const double len = std::sqrt(lx * lx + ly * ly + lz * lz);
    if (!(len > 0.0)) return fail(OW_ERR_INVALID, "light_direction has zero length");
    const double r = opts->roughness;
    for (int k = 0; k < 3; ++k) {
        sp->water_color[k] = opts->water_color[k];
        sp->foam_color[k] = opts->foam_color[k];
        sp->light[k] = (float)((double)opts->light_direction[k] / len);
        sp->light_color[k] = opts->light_color[k];
        sp->ambient_color[k] = opts->ambient_color[k];
        sp->sky_color[k] = opts->sky_color[k];
    }
    sp->roughness = opts->roughness;
    sp->normal_strength = opts->normal_strength;
    sp->fresnel_power = (float)(5.0 * std::exp(-2.69 * r));            // water.gdshader:92
    sp->fresnel_divisor = (float)(1.0 + 22.7 * std::pow(r, 1.5));      // water.gdshader:92
    return OW_OK;
}
}  // namespace ow::readside

namespace {
// the argument checks both forms of ow_render_view share, in this order: pointers, camera, options, context
ow_status check_render(const ow_context *c, const ow_camera *camera, const float *map_scales, int32_t num_cascades, const ow_render_options *opts,
                       const void *rgba, const void *pixels, ow::CameraParams *cp, ow::RaycastParams *rp, ow::ShadeParams *sp) {
    static_assert(sizeof(ow_render_pixel) == sizeof(ow::RenderPixel) && offsetof(ow_render_pixel, dist) == offsetof(ow::RenderPixel, dist) &&
                      offsetof(ow_render_pixel, normal) == offsetof(ow::RenderPixel, normal) &&
                      offsetof(ow_render_pixel, color) == offsetof(ow::RenderPixel, color) && OW_RENDER_MAX_SIDE == ow::kRenderMaxSide,
                  "record layout");
    if (!rgba && !pixels) return fail(OW_ERR_INVALID, "null argument: both outputs");
    if (!map_scales) return fail(OW_ERR_INVALID, "null argument");
    if (ow_status st = resolve_camera(camera, cp); st != OW_OK) return st;
    if (ow_status st = resolve_render_options(opts, rp, sp); st != OW_OK) return st;
    return check_point_query(c, 0, num_cascades);
}

// a view's launch on the context's stream (the bound words are there: ray_bound_words)
ow_status view_enqueue(ow_context *c, const ow::CameraParams &cp, const float *map_scales, int num_cascades, const ow::RaycastParams &rp,
                       const ow::ShadeParams &sp, uint32_t *rgba_dev, ow::RenderPixel *pixels_dev) {
    const ow::MapsView v = view_of(c);
    OW_HIP(ow::launch_render_view(v.n, num_cascades, v.buf, cp, surface_scales(map_scales, num_cascades), rp, sp, c->ray_bound, rgba_dev, pixels_dev, v.stream));
    return OW_OK;
}
}  // namespace

extern "C" {

void ow_render_options_default(ow_render_options *out) {
    if (out) render_defaults(out);
}

ow_status ow_render_view(ow_context *c, const ow_camera *camera, const float *map_scales, int32_t num_cascades, const ow_render_options *opts,
                         void *rgba8_out, ow_render_pixel *pixels_out) {
    ow::CameraParams cp;
    ow::RaycastParams rp;
    ow::ShadeParams sp;
    if (ow_status st = check_render(c, camera, map_scales, num_cascades, opts, rgba8_out, pixels_out, &cp, &rp, &sp); st != OW_OK) return st;
    OW_HIP(hipSetDevice(c->device));
    if (ow_status st = ray_bound_words(&c->ray_bound); st != OW_OK) return st;
    return picture_round_trip(c, (size_t)cp.width * cp.height, rgba8_out, pixels_out, false, layer_mask(num_cascades),
                              [&](uint32_t *rgba_dev, ow::RenderPixel *px_dev) { return view_enqueue(c, cp, map_scales, num_cascades, rp, sp, rgba_dev, px_dev); });
}

ow_status ow_render_view_async(ow_context *c, const ow_camera *camera, const float *map_scales, int32_t num_cascades, const ow_render_options *opts,
                               void *rgba8_dev, ow_render_pixel *pixels_dev) {
    ow::CameraParams cp;
    ow::RaycastParams rp;
    ow::ShadeParams sp;
    if (ow_status st = check_render(c, camera, map_scales, num_cascades, opts, rgba8_dev, pixels_dev, &cp, &rp, &sp); st != OW_OK) return st;
    if (ow_status st = check_pixel_alignment(rgba8_dev, pixels_dev); st != OW_OK) return st;
    if (ow_status st = begin_async(c, num_cascades); st != OW_OK) return st;
    if (ow_status st = ray_bound_words(&c->ray_bound); st != OW_OK) return st;
    return view_enqueue(c, cp, map_scales, num_cascades, rp, sp, (uint32_t *)rgba8_dev, (ow::RenderPixel *)pixels_dev);
}

}  // extern "C"

// ow_mirror_host.hip -- the floating bodies' reflections in the water: ow_mirror_options_init, ow_mirror_apply in its three forms and
// ow_mirror_stats over the kernel of ow_mirror.hip (ow_mirror.h).  The pass owns no handle: it reads a radiance pyramid (ow_sky_host.hip), a
// solid's shape with its cached sphere and a body set's resident poses (ow_solid_host.hip).
#include <cmath>
#include <cstring>

#include "ow_consumer_host.h"

using namespace ow::readside;
using ow::fail, ow::main_stream, ow::sync_stream;

namespace {
// the sky-light pass's defaults (ow_radiance_light_options_default) and the solid draw's (ow_solid_options_default); 200 m of mirror ray,
// the image fading out over the second hundred
void mirror_defaults(ow_mirror_options *o) {
    ow_solid_options so;
    ow_solid_options_default(&so);
    ow_radiance_light_options lo;
    ow_radiance_light_options_default(&lo);
    std::memset(o, 0, sizeof(*o));
    o->ambient_energy = lo.ambient_energy;
    o->reflection_energy = lo.reflection_energy;
    o->specular = lo.specular;
    for (int k = 0; k < 3; ++k) {
        o->body_color[k] = so.color[k];
        o->light_direction[k] = so.light_direction[k];
        o->light_color[k] = so.light_color[k];
        o->ambient_color[k] = so.ambient_color[k];
    }
    o->max_distance = ow::kMirrorDefaultDistance;
    o->fade_begin = ow::kMirrorDefaultFadeBegin;
    o->opacity = 1.0f;
}

// ow_mirror_options (NULL = ow_mirror_options_init's values) -> the pass's constants; the pyramid's are filled in by mirror_apply
ow_status resolve_mirror_options(const ow_mirror_options *opts, ow::SkyLightParams *lp, ow::MirrorParams *mp) {
    static_assert(sizeof(ow_mirror_options) == sizeof(ow::MirrorOptions) && offsetof(ow_mirror_options, body_color) == offsetof(ow::MirrorOptions, body_color) &&
                      offsetof(ow_mirror_options, light_direction) == offsetof(ow::MirrorOptions, light_direction) &&
                      offsetof(ow_mirror_options, ambient_color) == offsetof(ow::MirrorOptions, ambient_color) &&
                      offsetof(ow_mirror_options, max_distance) == offsetof(ow::MirrorOptions, max_distance) &&
                      offsetof(ow_mirror_options, opacity) == offsetof(ow::MirrorOptions, opacity) &&
                      offsetof(ow_mirror_options, flags) == offsetof(ow::MirrorOptions, flags) && offsetof(ow_mirror_options, cull) == offsetof(ow::MirrorOptions, cull) &&
                      offsetof(ow_mirror_options, reserved) == offsetof(ow::MirrorOptions, reserved) && OW_RAY_MIRROR == ow::kRayMirror &&
                      OW_MIRROR_TWO_SIDED == ow::kMirrorTwoSided,
                  "record layout");
    ow_mirror_options def;
    opts = or_defaults(opts, &def, mirror_defaults);
    std::memset(lp, 0, sizeof(*lp));
    std::memset(mp, 0, sizeof(*mp));
    if (!in_range(opts->ambient_energy, 0.0f, ow::kSkyLightEnergyMax)) return fail(OW_ERR_INVALID, "ow_mirror_options: ambient_energy outside [0,1e12]");
    if (!in_range(opts->reflection_energy, 0.0f, ow::kSkyLightEnergyMax)) return fail(OW_ERR_INVALID, "ow_mirror_options: reflection_energy outside [0,1e12]");
    if (!in_range(opts->specular, 0.0f, 1.0f)) return fail(OW_ERR_INVALID, "ow_mirror_options: specular outside [0,1]");
    const float *vec[4] = {opts->body_color, opts->light_direction, opts->light_color, opts->ambient_color};
    for (const float *v : vec)
        for (int k = 0; k < 3; ++k)
            if (!(std::fabs(v[k]) <= ow::kSolidColorMax)) return fail(OW_ERR_INVALID, "ow_mirror_options: a colour or the light direction is not finite (or beyond 1e12)");
    if (!(opts->max_distance > 0.0f) || !in_range(opts->max_distance, 0.0f, ow::kMirrorDistanceMax))
        return fail(OW_ERR_INVALID, "ow_mirror_options: max_distance outside (0,1e12]");
    if (!in_range(opts->fade_begin, 0.0f, opts->max_distance) || !(opts->fade_begin < opts->max_distance))
        return fail(OW_ERR_INVALID, "ow_mirror_options: fade_begin outside [0,max_distance)");
    if (!in_range(opts->opacity, 0.0f, 1.0f)) return fail(OW_ERR_INVALID, "ow_mirror_options: opacity outside [0,1]");
    if (opts->flags & ~OW_MIRROR_TWO_SIDED) return fail(OW_ERR_INVALID, "unknown mirror flags 0x%x", opts->flags);
    if (opts->cull != 0 && opts->cull != -1) return fail(OW_ERR_INVALID, "cull %d is neither 0 nor -1", opts->cull);
    if (ow_status st = check_reserved(opts->reserved, "ow_mirror_options"); st != OW_OK) return st;
    const double lx = opts->light_direction[0], ly = opts->light_direction[1], lz = opts->light_direction[2];
    const double len = std::sqrt(lx * lx + ly * ly + lz * lz);
    if (!(len > 0.0)) return fail(OW_ERR_INVALID, "light_direction has zero length");
    lp->ambient_energy = opts->ambient_energy;
    lp->reflection_energy = opts->reflection_energy;
    ow::sky_light_fresnel(opts->specular, lp->f0, lp->f50);
    lp->camera_ok = 1;
    for (int k = 0; k < 3; ++k) {
        mp->body_color[k] = opts->body_color[k];
        mp->light[k] = (float)((double)opts->light_direction[k] / len);
        mp->light_color[k] = opts->light_color[k];
        mp->ambient_color[k] = opts->ambient_color[k];
    }
    mp->max_distance = opts->max_distance;
    mp->fade_begin = opts->fade_begin;
    mp->opacity = opts->opacity;
    mp->cp.two_sided = (opts->flags & OW_MIRROR_TWO_SIDED) ? 1 : 0;
    mp->cp.cull = opts->cull == 0 ? 1 : 0;
    return OW_OK;
}

enum class Form { kHost, kAsync, kInstances };

// The pass in its three forms.  The argument checks: ow_radiance_light_apply's, in its order (the records, the camera, the options, the
// context and the pyramid), then the shape, the set and the ranges as ow_cast_bodies checks them.  The synchronous forms keep the
// records in the context's pixel block and the hit records in the pass's scratch.
ow_status mirror_apply(ow_context *c, Form form, const ow_radiance *radiance, ow_solid *solid, const ow_bodies *set, int32_t first, const float *upload,
                       int32_t instances, const ow_camera *camera, const ow_mirror_options *opts, ow_render_pixel *pixels, ow_solid_hit *hits) {
    ow::CameraParams cp;
    ow::SkyLightParams lp;
    ow::MirrorParams mp;
    if (!pixels) return fail(OW_ERR_INVALID, "null argument: the records");
    if (ow_status st = resolve_camera(camera, &cp); st != OW_OK) return st;
    if (ow_status st = resolve_mirror_options(opts, &lp, &mp); st != OW_OK) return st;
    if (form == Form::kInstances) {
        if (instances < 0 || instances > OW_SOLID_MAX_INSTANCES) return fail(OW_ERR_INVALID, "instance_count %d outside [0,%d]", instances, OW_SOLID_MAX_INSTANCES);
        if (instances > 0 && !upload) return fail(OW_ERR_INVALID, "null argument");
    }
    if (ow_status st = check_handle(c, radiance, "radiance pyramid"); st != OW_OK) return st;
    if (solid) {
        if (ow_status st = check_handle(c, solid, "solid"); st != OW_OK) return st;
        if (form == Form::kInstances) {
            if (ow_status st = check_solid_count(solid, instances); st != OW_OK) return st;
        } else if (set || instances != 0) {
            if (ow_status st = check_solid_bodies(c, solid, set, first, instances); st != OW_OK) return st;
        }
    } else if (instances != 0) {
        return fail(OW_ERR_INVALID, "null argument: a solid is required with %d instances", instances);
    }
    const bool async = form == Form::kAsync;
    if (async) {
        if (ow_status st = check_pixel_alignment(nullptr, pixels); st != OW_OK) return st;
        if ((uintptr_t)hits & 3u) return fail(OW_ERR_INVALID, "hits_dev must be 4-byte aligned");
    }
    lp.levels = radiance->plan.levels;
    for (int k = 0; k < radiance->plan.levels; ++k) lp.R[k] = radiance->R[k];
    lp.E = radiance->E;
    lp.camera_ok = ow::mesh_camera_ok(cp) ? 1 : 0;

    OW_HIP(hipSetDevice(c->device));
    const size_t count = (size_t)cp.width * cp.height;
    Layout L;
    L.take(ow::kMirrorCounterBytes);  // the counters, at 0
    const size_t b_off = L.take((size_t)instances * sizeof(ow::SolidCastBound));
    const size_t t_off = L.take(instance_upload_bytes(upload, instances));
    const size_t h_off = L.take(!async && hits ? count * sizeof(ow::SolidHit) : 0);
    if (ow_status st = sync_before_growth(c, c->mirror, L.total); st != OW_OK) return st;
    if (ow_status st = c->mirror.ensure(L.total, 0, 1, "bytes of mirror scratch"); st != OW_OK) return st;
    char *base = (char *)c->mirror.ptr;
    hipStream_t s = main_stream(c);
    ow::RenderPixel *pixels_dev = (ow::RenderPixel *)pixels;
    ow::SolidHit *hits_dev = (ow::SolidHit *)hits;
    if (!async) {
        if (ow_status st = c->render_pixels.ensure(count * sizeof(ow::RenderPixel), 0, sizeof(ow::RenderPixel), "pixel records"); st != OW_OK) return st;
        pixels_dev = (ow::RenderPixel *)c->render_pixels.ptr;
        hits_dev = hits ? (ow::SolidHit *)(base + h_off) : nullptr;
        OW_HIP(hipMemcpyAsync(pixels_dev, pixels, count * sizeof(ow::RenderPixel), hipMemcpyHostToDevice, s));
    }
    ow::MirrorArrays A{};
    A.counters = base;
    A.bounds = (ow::SolidCastBound *)(base + b_off);
    ow::SolidInstances in{nullptr, nullptr, ow::kSolidTransformFloats, 0};
    if (solid && instances > 0) {
        if (!solid->bound_enqueued) {  // once per shape, in stream order ahead of everything that reads it
            OW_HIP(ow::launch_solid_cast_shape_bound(solid->shape, solid->bound, s));
            solid->bound_enqueued = true;
        }
        A.shape = solid->shape;
        A.shape_bound = solid->bound;
        if (ow_status st = instance_source(set, first, upload, instances, base + t_off, s, &in); st != OW_OK) return st;
    }
    OW_HIP(ow::launch_mirror_apply(A, in, cp, lp, mp, pixels_dev, hits_dev, s));
    ++c->mirror_passes;
    if (async) return OW_OK;
    OW_HIP(hipMemcpyAsync(pixels, pixels_dev, count * sizeof(ow::RenderPixel), hipMemcpyDeviceToHost, s));
    if (hits) OW_HIP(hipMemcpyAsync(hits, hits_dev, count * sizeof(ow::SolidHit), hipMemcpyDeviceToHost, s));
    return sync_stream(c, 0);
}
}  // namespace

extern "C" {

void ow_mirror_options_init(ow_mirror_options *out) {
    if (out) mirror_defaults(out);
}

ow_status ow_mirror_apply(ow_context *c, ow_radiance *radiance, ow_solid *solid, ow_bodies *bodies, int32_t first_body, int32_t body_count,
                          const ow_camera *camera, const ow_mirror_options *opts, ow_render_pixel *pixels_inout, ow_solid_hit *hits_out) {
    return mirror_apply(c, Form::kHost, radiance, solid, bodies, first_body, nullptr, body_count, camera, opts, pixels_inout, hits_out);
}

ow_status ow_mirror_apply_async(ow_context *c, ow_radiance *radiance, ow_solid *solid, ow_bodies *bodies, int32_t first_body, int32_t body_count,
                                const ow_camera *camera, const ow_mirror_options *opts, ow_render_pixel *pixels_dev, ow_solid_hit *hits_dev) {
    return mirror_apply(c, Form::kAsync, radiance, solid, bodies, first_body, nullptr, body_count, camera, opts, pixels_dev, hits_dev);
}

ow_status ow_mirror_apply_instances(ow_context *c, ow_radiance *radiance, ow_solid *solid, const float *transforms, int32_t instance_count,
                                    const ow_camera *camera, const ow_mirror_options *opts, ow_render_pixel *pixels_inout, ow_solid_hit *hits_out) {
    return mirror_apply(c, Form::kInstances, radiance, solid, nullptr, 0, transforms, instance_count, camera, opts, pixels_inout, hits_out);
}

ow_status ow_mirror_stats(ow_context *c, uint64_t *passes, uint64_t *pixels, uint64_t *rays_cast, uint64_t *sphere_tests_passed, uint64_t *pairs_tested,
                          uint64_t *rays_hit) {
    if (!c) return fail(OW_ERR_INVALID, "null context");
    uint64_t n[ow::kMirrorCounters] = {0, 0, 0, 0, 0};  // no pass yet, no scratch: zeros, and the device is not touched
    if (c->mirror.ptr && (pixels || rays_cast || sphere_tests_passed || pairs_tested || rays_hit)) {
        alignas(8) unsigned char head[ow::kMirrorCounterBytes];
        OW_HIP(hipSetDevice(c->device));
        if (ow_status st = read_back(c, head, c->mirror.ptr, sizeof(head)); st != OW_OK) return st;
        for (int slot = 0; slot < ow::kMirrorSlots; ++slot) {
            uint64_t copy[ow::kMirrorCounters];
            std::memcpy(copy, head + ow::kMirrorSumsOffset + (size_t)slot * ow::kMirrorSlotWords * sizeof(uint64_t), sizeof(copy));
            for (int k = 0; k < ow::kMirrorCounters; ++k) n[k] += copy[k];
        }
    }
    if (passes) *passes = c->mirror_passes;
    if (pixels) *pixels = n[ow::kMirrorPixels];
    if (rays_cast) *rays_cast = n[ow::kMirrorRays];
    if (sphere_tests_passed) *sphere_tests_passed = n[ow::kMirrorPassed];
    if (pairs_tested) *pairs_tested = n[ow::kMirrorPairs];
    if (rays_hit) *rays_hit = n[ow::kMirrorHits];
    return OW_OK;
}

}  // extern "C"

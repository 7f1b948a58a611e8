// ow_mist_host.hip -- the height mist with sun shafts: ow_mist_options_init, ow_mist_apply in both forms and ow_mist_stats over the kernel of
// ow_mist.hip (ow_mist.h).  The pass owns no handle: it reads a shadow map (ow_solid_host.hip) where it is given one.
#include <cmath>
#include <cstring>

#include "ow_consumer_host.h"

using namespace ow::readside;
using ow::fail, ow::main_stream;

namespace {
// main.tscn:35-37 (length 256), :100-104 and :142-144 (the FogVolume's FogMaterial: height_falloff 0.176, its albedo), the Sun's +Z axis
// (:113) with a white sun of energy 1 as ow_render_options_default's light; the engine's defaults for anisotropy (0.2) and sky affect (1).
// main.tscn:101's density 8.0 is in an engine unit whose scale the reference does not carry: extinction 0.02 / m is this library's choice
// (half of a 35 m path at sea level is mist).
void mist_defaults(ow_mist_options *o) {
    ow_render_options ro;
    render_defaults(&ro);
    std::memset(o, 0, sizeof(*o));
    o->extinction = 0.02f;
    o->height_falloff = 0.176f;
    o->base_height = 0.0f;
    o->length = 256.0f;
    o->anisotropy = 0.2f;
    o->sky_affect = 1.0f;
    o->slices = ow::kMistDefaultSlices;
    o->shadow_bias = 0.0f;
    const float albedo[3] = {0.988718f, 0.989631f, 0.989629f};
    for (int k = 0; k < 3; ++k) {
        o->albedo[k] = albedo[k];
        o->sun_color[k] = ro.light_color[k];
        o->sun_direction[k] = ro.light_direction[k];
        o->ambient_color[k] = ro.ambient_color[k];
    }
}

// ow_mist_options (NULL = ow_mist_options_init's values) -> the pass's constants
ow_status resolve_mist_options(const ow_mist_options *opts, ow::MistParams *mp) {
    static_assert(sizeof(ow_mist_options) == sizeof(ow::MistOptions) && offsetof(ow_mist_options, slices) == offsetof(ow::MistOptions, slices) &&
                      offsetof(ow_mist_options, shadow_bias) == offsetof(ow::MistOptions, shadow_bias) &&
                      offsetof(ow_mist_options, albedo) == offsetof(ow::MistOptions, albedo) &&
                      offsetof(ow_mist_options, ambient_color) == offsetof(ow::MistOptions, ambient_color) &&
                      offsetof(ow_mist_options, reserved) == offsetof(ow::MistOptions, reserved) && OW_RAY_MIST == ow::kRayMist &&
                      OW_MIST_MAX_SLICES == ow::kMistMaxSlices,
                  "record layout");
    ow_mist_options def;
    opts = or_defaults(opts, &def, mist_defaults);
    if (!in_range(opts->extinction, 0.0f, ow::kMistExtinctionMax)) return fail(OW_ERR_INVALID, "ow_mist_options: extinction outside [0,1e3]");
    if (!in_range(opts->height_falloff, 0.0f, ow::kMistFalloffMax)) return fail(OW_ERR_INVALID, "ow_mist_options: height_falloff outside [0,1e3]");
    if (!in_range(opts->base_height, -ow::kMistRangeMax, ow::kMistRangeMax)) return fail(OW_ERR_INVALID, "ow_mist_options: base_height outside [-1e6,1e6]");
    if (!in_range(opts->length, 0.0f, ow::kMistRangeMax)) return fail(OW_ERR_INVALID, "ow_mist_options: length outside [0,1e6]");
    if (!in_range(opts->anisotropy, -ow::kMistAnisotropyMax, ow::kMistAnisotropyMax)) return fail(OW_ERR_INVALID, "ow_mist_options: anisotropy outside [-0.9,0.9]");
    if (!in_range(opts->sky_affect, 0.0f, 1.0f)) return fail(OW_ERR_INVALID, "ow_mist_options: sky_affect outside [0,1]");
    if (opts->slices < 0 || opts->slices > OW_MIST_MAX_SLICES) return fail(OW_ERR_INVALID, "slices %d outside [0,%d]", opts->slices, OW_MIST_MAX_SLICES);
    if (opts->flags != 0u) return fail(OW_ERR_INVALID, "unknown mist flags 0x%x", opts->flags);
    if (!in_range(opts->shadow_bias, -ow::kMistRangeMax, ow::kMistRangeMax)) return fail(OW_ERR_INVALID, "ow_mist_options: shadow_bias outside [-1e6,1e6]");
    const float *colors[3] = {opts->albedo, opts->sun_color, opts->ambient_color};
    for (const float *v : colors)
        for (int k = 0; k < 3; ++k)
            if (!in_range(v[k], 0.0f, ow::kMistColorMax)) return fail(OW_ERR_INVALID, "ow_mist_options: a colour channel outside [0,1e6]");
    for (int k = 0; k < 3; ++k)
        if (!(std::fabs(opts->sun_direction[k]) <= ow::kMistRangeMax)) return fail(OW_ERR_INVALID, "ow_mist_options: sun_direction is not finite (or beyond 1e6)");
    if (ow_status st = check_reserved(opts->reserved, "ow_mist_options"); st != OW_OK) return st;
    ow::MistOptions mo;
    std::memcpy(&mo, opts, sizeof(mo));
    if (!ow::mist_params(mo, true, mp)) return fail(OW_ERR_INVALID, "sun_direction has zero length");
    return OW_OK;
}

// The pass in either form (pixel_pass).  The argument checks both forms share: ow_shadow_apply's, in its order, then the context and the map.
ow_status mist_apply(ow_context *c, bool async, const ow_shadow_map *map, const ow_camera *camera, const ow_mist_options *opts, ow_render_pixel *pixels, void *rgba8) {
    ow::CameraParams cp;
    ow::MistParams mp;
    if (!pixels) return fail(OW_ERR_INVALID, "null argument: the records");
    if (ow_status st = resolve_camera(camera, &cp); st != OW_OK) return st;
    if (ow_status st = resolve_mist_options(opts, &mp); st != OW_OK) return st;
    if (!c) return fail(OW_ERR_INVALID, "null context");
    if (map)
        if (ow_status st = check_handle(c, map, "shadow map"); st != OW_OK) return st;
    mp.camera_ok = ow::mesh_camera_ok(cp) ? 1 : 0;
    const bool shafts = map && map->P.ok;     // a map that has had no ow_shadow_map_begin shadows nothing
    ow::ShadowParams P{};
    if (shafts) P = map->P;
    if (async)
        if (ow_status st = check_pixel_alignment(rgba8, pixels); st != OW_OK) return st;
    OW_HIP(hipSetDevice(c->device));
    if (ow_status st = c->mist.ensure(ow::kMistCounterBytes, 0, 1, "bytes of mist counters"); st != OW_OK) return st;
    const ow_status st = pixel_pass(c, async, (size_t)cp.width * cp.height, rgba8, pixels, [&](uint32_t *rgba_dev, ow::RenderPixel *pixels_dev) {
        OW_HIP(ow::launch_mist_apply(shafts ? map->map : nullptr, cp, P, mp, pixels_dev, rgba_dev, (unsigned long long *)c->mist.ptr, main_stream(c)));
        return OW_OK;
    });
    if (st == OW_OK) ++c->mist_passes;
    return st;
}
}  // namespace

extern "C" {

void ow_mist_options_init(ow_mist_options *out) {
    if (out) mist_defaults(out);
}

ow_status ow_mist_apply(ow_context *c, ow_shadow_map *map, const ow_camera *camera, const ow_mist_options *opts, ow_render_pixel *pixels_inout, void *rgba8_out) {
    return mist_apply(c, false, map, camera, opts, pixels_inout, rgba8_out);
}

ow_status ow_mist_apply_async(ow_context *c, ow_shadow_map *map, const ow_camera *camera, const ow_mist_options *opts, ow_render_pixel *pixels_dev, void *rgba8_dev) {
    return mist_apply(c, true, map, camera, opts, pixels_dev, rgba8_dev);
}

ow_status ow_mist_stats(ow_context *c, uint64_t *passes, uint64_t *pixels, uint64_t *slices_fetched, uint64_t *slices_shadowed) {
    if (!c) return fail(OW_ERR_INVALID, "null context");
    unsigned long long n[ow::kMistCounters] = {0, 0, 0};
    if ((pixels || slices_fetched || slices_shadowed) && c->mist_passes > 0) {   // before the first pass there are no counters
        static_assert(ow::kMistCounters <= ow::kMistCounterStride, "a copy of the counters fits its line");
        unsigned long long copies[ow::kMistCounterSlots * ow::kMistCounterStride];
        if (ow_status st = read_back(c, copies, c->mist.ptr, sizeof(copies)); st != OW_OK) return st;
        for (int slot = 0; slot < ow::kMistCounterSlots; ++slot)
            for (int k = 0; k < ow::kMistCounters; ++k) n[k] += copies[slot * ow::kMistCounterStride + k];
    }
    if (passes) *passes = c->mist_passes;
    if (pixels) *pixels = n[ow::kMistPixels];
    if (slices_fetched) *slices_fetched = n[ow::kMistFetched];
    if (slices_shadowed) *slices_shadowed = n[ow::kMistShadowed];
    return OW_OK;
}

}  // extern "C"

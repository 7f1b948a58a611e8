// ow_sky_host.hip -- what finishes a picture: the ow_sky_* panoramas, ow_environment_apply and ow_present over the kernels of
// ow_environment.hip (ow_environment.h), and the light from the sky, the ow_radiance_* pyramids and their pass, over those of
// ow_sky_light.hip (ow_sky_light.h).
#include <cmath>
#include <cstring>
#include <vector>

#include "ow_consumer_host.h"

using namespace ow::readside;
using ow::fail, ow::main_stream, ow::sync_stream;

/* ---- the environment pass and the present (ow_environment.h, ow_environment.hip) ---- */

namespace {
void sky_defaults(ow_sky_options *o) {
    std::memset(o, 0, sizeof(*o));
    o->srgb = 1u;
    o->energy = 1.0f;
}
// main.tscn:22-41 and the Sun's +Z axis (:113), a white sun of energy 1 as ow_render_options_default's light
void environment_defaults(ow_environment_options *o) {
    ow_render_options ro;
    render_defaults(&ro);
    std::memset(o, 0, sizeof(*o));
    o->fog_mode = OW_FOG_DEPTH;
    o->density = 1.0f;
    o->depth_begin = 200.0f;
    o->depth_end = 350.0f;
    o->depth_curve = 0.25f;
    o->aerial_perspective = 0.626f;
    o->sun_scatter = 0.05f;
    const float fog[3] = {0.272954f, 0.419272f, 0.484632f};
    for (int k = 0; k < 3; ++k) {
        o->light_color[k] = fog[k];
        o->sun_color[k] = ro.light_color[k];
        o->sun_direction[k] = ro.light_direction[k];
        o->sky_color[k] = ro.sky_color[k];
    }
}
void present_defaults(ow_present_options *o) {
    std::memset(o, 0, sizeof(*o));
    o->downsample = 1;
    o->tonemap = OW_TONEMAP_FILMIC;
    o->exposure = 1.0f;
    o->white = 1.0f;
    o->srgb = 1u;
    o->brightness = 0.85f;
    o->contrast = 1.07f;
    o->saturation = 1.5f;
}

ow_status check_sky_options(const ow_sky_options *o) {
    static_assert(sizeof(ow_sky_options) == sizeof(ow::SkyOptions) && offsetof(ow_sky_options, energy) == offsetof(ow::SkyOptions, energy) &&
                      OW_SKY_MAX_SIDE == ow::kSkyMaxSide,
                  "record layout");
    if (o->srgb > 1u) return fail(OW_ERR_INVALID, "ow_sky_options: srgb is not 0 or 1");
    if (!in_range(o->energy, 0.0f, ow::kEnvColorMax)) return fail(OW_ERR_INVALID, "ow_sky_options: energy outside [0,1e12]");
    return check_reserved(o->reserved, "ow_sky_options");
}

// ow_environment_options (NULL = the defaults) -> the pass's constants; the sky's are filled in by environment_apply
ow_status resolve_environment_options(const ow_environment_options *opts, ow::EnvParams *ep) {
    static_assert(sizeof(ow_environment_options) == sizeof(ow::EnvironmentOptions) &&
                      offsetof(ow_environment_options, flags) == offsetof(ow::EnvironmentOptions, flags) &&
                      offsetof(ow_environment_options, sun_direction) == offsetof(ow::EnvironmentOptions, sun_direction) &&
                      offsetof(ow_environment_options, reserved) == offsetof(ow::EnvironmentOptions, reserved) && OW_RAY_ENVIRONMENT == ow::kRayEnvironment &&
                      OW_FOG_EXPONENTIAL == ow::kFogExponential && OW_FOG_DEPTH == ow::kFogDepth,
                  "record layout");
    ow_environment_options def;
    opts = or_defaults(opts, &def, environment_defaults);
    std::memset(ep, 0, sizeof(*ep));
    if (opts->fog_mode != OW_FOG_EXPONENTIAL && opts->fog_mode != OW_FOG_DEPTH) return fail(OW_ERR_INVALID, "unknown fog_mode %d", opts->fog_mode);
    if (!in_range(opts->density, 0.0f, ow::kEnvColorMax)) return fail(OW_ERR_INVALID, "ow_environment_options: density outside [0,1e12]");
    if (!in_range(opts->depth_begin, 0.0f, ow::kEnvColorMax) || !in_range(opts->depth_end, opts->depth_begin, ow::kEnvColorMax))
        return fail(OW_ERR_INVALID, "ow_environment_options: depth_begin and depth_end must satisfy 0 <= begin <= end <= 1e12");
    if (!in_range(opts->depth_curve, ow::kEnvCurveMin, ow::kEnvCurveMax)) return fail(OW_ERR_INVALID, "ow_environment_options: depth_curve outside [0.01,100]");
    if (!in_range(opts->aerial_perspective, 0.0f, 1.0f)) return fail(OW_ERR_INVALID, "ow_environment_options: aerial_perspective outside [0,1]");
    if (!in_range(opts->sun_scatter, 0.0f, ow::kEnvColorMax)) return fail(OW_ERR_INVALID, "ow_environment_options: sun_scatter outside [0,1e12]");
    const float *vec[4] = {opts->light_color, opts->sun_color, opts->sun_direction, opts->sky_color};
    for (const float *v : vec)
        for (int k = 0; k < 3; ++k)
            if (!(std::fabs(v[k]) <= ow::kEnvColorMax)) return fail(OW_ERR_INVALID, "ow_environment_options: a colour or the sun direction is not finite (or beyond 1e12)");
    if (opts->flags != 0u) return fail(OW_ERR_INVALID, "unknown environment flags 0x%x", opts->flags);
    if (ow_status st = check_reserved(opts->reserved, "ow_environment_options"); st != OW_OK) return st;
    const double lx = opts->sun_direction[0], ly = opts->sun_direction[1], lz = opts->sun_direction[2];
    const double len = std::sqrt(lx * lx + ly * ly + lz * lz);
    if (!(len > 0.0)) return fail(OW_ERR_INVALID, "sun_direction has zero length");
    ep->fog_mode = opts->fog_mode;
    ep->density = opts->density;
    ep->begin = opts->depth_begin;
    ep->end = opts->depth_end;
    ep->curve = opts->depth_curve;
    ep->aerial = opts->aerial_perspective;
    ep->scatter = opts->sun_scatter;
    for (int k = 0; k < 3; ++k) {
        ep->light_color[k] = opts->light_color[k];
        ep->sun_color[k] = opts->sun_color[k];
        ep->sun[k] = (float)((double)opts->sun_direction[k] / len);
        ep->sky_color[k] = opts->sky_color[k];
    }
    ep->camera_ok = 1;
    ep->energy = 1.0f;
    return OW_OK;
}

// The pass in either form (pixel_pass).  The argument checks both forms share: ow_solid_draw's, in its order, then the context and the sky.
ow_status environment_apply(ow_context *c, bool async, const ow_sky *sky, const ow_camera *camera, const ow_environment_options *opts, ow_render_pixel *pixels) {
    ow::CameraParams cp;
    ow::EnvParams ep;
    if (!pixels) return fail(OW_ERR_INVALID, "null argument: the records");
    if (ow_status st = resolve_camera(camera, &cp); st != OW_OK) return st;
    if (ow_status st = resolve_environment_options(opts, &ep); st != OW_OK) return st;
    if (!c) return fail(OW_ERR_INVALID, "null context");
    if (sky) {
        if (ow_status st = check_handle(c, sky, "sky"); st != OW_OK) return st;
        ep.has_sky = 1;
        ep.sky = sky->tex;
        ep.srgb = sky->srgb;
        ep.energy = sky->energy;
    }
    ep.camera_ok = ow::mesh_camera_ok(cp) ? 1 : 0;
    return pixel_pass(c, async, (size_t)cp.width * cp.height, nullptr, pixels, [&](uint32_t *, ow::RenderPixel *pixels_dev) {
        OW_HIP(ow::launch_environment_apply(cp, ep, pixels_dev, main_stream(c)));
        return OW_OK;
    });
}

// ow_present_options (NULL = the defaults) -> the present's constants and the output's size
ow_status resolve_present_options(const ow_present_options *opts, const ow::CameraParams &cp, ow::PresentParams *pp, int *out_width, int *out_height) {
    static_assert(sizeof(ow_present_options) == sizeof(ow::PresentOptions) && offsetof(ow_present_options, srgb) == offsetof(ow::PresentOptions, srgb) &&
                      offsetof(ow_present_options, reserved) == offsetof(ow::PresentOptions, reserved) &&
                      OW_PRESENT_MAX_DOWNSAMPLE == ow::kPresentMaxDownsample && OW_TONEMAP_LINEAR == ow::kTonemapLinear &&
                      OW_TONEMAP_REINHARD == ow::kTonemapReinhard && OW_TONEMAP_FILMIC == ow::kTonemapFilmic,
                  "record layout");
    ow_present_options def;
    opts = or_defaults(opts, &def, present_defaults);
    if (opts->downsample < 0 || opts->downsample > OW_PRESENT_MAX_DOWNSAMPLE)
        return fail(OW_ERR_INVALID, "downsample %d outside [0,%d]", opts->downsample, OW_PRESENT_MAX_DOWNSAMPLE);
    const int s = opts->downsample == 0 ? 1 : opts->downsample;
    if (cp.width % s != 0 || cp.height % s != 0) return fail(OW_ERR_INVALID, "downsample %d does not divide %d x %d", s, cp.width, cp.height);
    if (opts->tonemap < OW_TONEMAP_LINEAR || opts->tonemap > OW_TONEMAP_FILMIC) return fail(OW_ERR_INVALID, "unknown tonemap %d", opts->tonemap);
    if (!in_range(opts->exposure, 0.0f, ow::kPresentScaleMax)) return fail(OW_ERR_INVALID, "ow_present_options: exposure outside [0,1e6]");
    if (!in_range(opts->white, ow::kPresentWhiteMin, ow::kPresentScaleMax)) return fail(OW_ERR_INVALID, "ow_present_options: white outside [0.01,1e6]");
    if (opts->srgb > 1u) return fail(OW_ERR_INVALID, "ow_present_options: srgb is not 0 or 1");
    if (!in_range(opts->brightness, 0.0f, ow::kPresentAdjustMax) || !in_range(opts->contrast, 0.0f, ow::kPresentAdjustMax) ||
        !in_range(opts->saturation, 0.0f, ow::kPresentAdjustMax))
        return fail(OW_ERR_INVALID, "ow_present_options: brightness, contrast or saturation outside [0,8]");
    if (opts->flags != 0u) return fail(OW_ERR_INVALID, "unknown present flags 0x%x", opts->flags);
    if (ow_status st = check_reserved(opts->reserved, "ow_present_options"); st != OW_OK) return st;
    pp->s = s;
    pp->inv = 1.0f / (float)(s * s);
    pp->tonemap = opts->tonemap;
    pp->exposure = opts->exposure;
    pp->white = opts->white;
    pp->srgb = (int)opts->srgb;
    pp->brightness = opts->brightness;
    pp->contrast = opts->contrast;
    pp->saturation = opts->saturation;
    *out_width = cp.width / s;
    *out_height = cp.height / s;
    return OW_OK;
}

// the argument checks both forms of the present share: outputs and records, camera, options, context
ow_status check_present(const ow_context *c, const ow_camera *camera, const ow_present_options *opts, const void *pixels, const void *rgba, const void *linear,
                        ow::CameraParams *cp, ow::PresentParams *pp, int *out_width, int *out_height) {
    if (!rgba && !linear) return fail(OW_ERR_INVALID, "null argument: both outputs");
    if (!pixels) return fail(OW_ERR_INVALID, "null argument: the records");
    if (ow_status st = resolve_camera(camera, cp); st != OW_OK) return st;
    if (ow_status st = resolve_present_options(opts, *cp, pp, out_width, out_height); st != OW_OK) return st;
    if (!c) return fail(OW_ERR_INVALID, "null context");
    return OW_OK;
}
}  // namespace

extern "C" {

void ow_sky_options_default(ow_sky_options *out) {
    if (out) sky_defaults(out);
}
void ow_environment_options_default(ow_environment_options *out) {
    if (out) environment_defaults(out);
}
void ow_present_options_default(ow_present_options *out) {
    if (out) present_defaults(out);
}

ow_status ow_sky_create(ow_context *c, const ow_sky_options *opts, const void *rgba8, int32_t width, int32_t height, ow_sky **out) {
    if (!out) return fail(OW_ERR_INVALID, "null argument");
    ow_sky_options def;
    opts = or_defaults(opts, &def, sky_defaults);
    if (width < 1 || width > OW_SKY_MAX_SIDE || height < 1 || height > OW_SKY_MAX_SIDE)
        return fail(OW_ERR_INVALID, "panorama size %d x %d outside [1,%d]", width, height, OW_SKY_MAX_SIDE);
    if (ow_status st = check_sky_options(opts); st != OW_OK) return st;
    if (!rgba8) return fail(OW_ERR_INVALID, "null argument");
    if (!c) return fail(OW_ERR_INVALID, "null context");
    float table[256];
    ow::spray_srgb_table(table);
    const size_t bytes = (size_t)width * height * 4;
    Layout L;
    const size_t t_off = L.take(sizeof(table)), p_off = L.take(bytes);
    ow_sky *sky;
    if (ow_status st = new_handle(c, L.total, "panorama", &sky); st != OW_OK) return st;
    char *base = (char *)sky->block;
    sky->srgb = (const float *)(base + t_off);
    sky->tex = ow::SprayTexture{(const uint32_t *)(base + p_off), width, height, (int)opts->srgb};
    sky->energy = opts->energy;
    hipStream_t s = main_stream(c);
    const bool enqueued = hipMemcpyAsync((void *)sky->srgb, table, sizeof(table), hipMemcpyHostToDevice, s) == hipSuccess &&
                          hipMemcpyAsync((void *)sky->tex.texels, rgba8, bytes, hipMemcpyHostToDevice, s) == hipSuccess;
    return finish_create(c, sky, s, enqueued, "panorama upload", out);
}

void ow_sky_destroy(ow_context *, ow_sky *sky) {
    if (sky) release_handle(sky);
    delete sky;
}

ow_status ow_environment_apply(ow_context *c, ow_sky *sky, const ow_camera *camera, const ow_environment_options *opts, ow_render_pixel *pixels_inout) {
    return environment_apply(c, false, sky, camera, opts, pixels_inout);
}

ow_status ow_environment_apply_async(ow_context *c, ow_sky *sky, const ow_camera *camera, const ow_environment_options *opts, ow_render_pixel *pixels_dev) {
    return environment_apply(c, true, sky, camera, opts, pixels_dev);
}

ow_status ow_present(ow_context *c, const ow_camera *camera, const ow_present_options *opts, const ow_render_pixel *pixels_in, void *rgba8_out,
                     float *linear_out) {
    ow::CameraParams cp;
    ow::PresentParams pp;
    int ow_ = 0, oh = 0;
    if (ow_status st = check_present(c, camera, opts, pixels_in, rgba8_out, linear_out, &cp, &pp, &ow_, &oh); st != OW_OK) return st;
    OW_HIP(hipSetDevice(c->device));
    const size_t in_count = (size_t)cp.width * cp.height, out_count = (size_t)ow_ * oh;
    if (ow_status st = c->render_pixels.ensure(in_count * sizeof(ow::RenderPixel), 0, sizeof(ow::RenderPixel), "pixel records"); st != OW_OK) return st;
    if (ow_status st = c->render_rgba.ensure(out_count * (4 * sizeof(float) + sizeof(uint32_t)), 0, sizeof(uint32_t), "pixels"); st != OW_OK) return st;
    hipStream_t s = main_stream(c);
    ow::RenderPixel *pixels_dev = (ow::RenderPixel *)c->render_pixels.ptr;
    float *linear_dev = (float *)c->render_rgba.ptr;
    uint32_t *rgba_dev = (uint32_t *)(linear_dev + 4 * out_count);
    OW_HIP(hipMemcpyAsync(pixels_dev, pixels_in, in_count * sizeof(ow::RenderPixel), hipMemcpyHostToDevice, s));
    OW_HIP(ow::launch_present(ow_, oh, pp, pixels_dev, rgba8_out ? rgba_dev : nullptr, linear_out ? linear_dev : nullptr, s));
    if (rgba8_out) OW_HIP(hipMemcpyAsync(rgba8_out, rgba_dev, out_count * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (linear_out) OW_HIP(hipMemcpyAsync(linear_out, linear_dev, out_count * 4 * sizeof(float), hipMemcpyDeviceToHost, s));
    return sync_stream(c, 0);
}

ow_status ow_present_async(ow_context *c, const ow_camera *camera, const ow_present_options *opts, const ow_render_pixel *pixels_dev, void *rgba8_dev,
                           float *linear_dev) {
    ow::CameraParams cp;
    ow::PresentParams pp;
    int ow_ = 0, oh = 0;
    if (ow_status st = check_present(c, camera, opts, pixels_dev, rgba8_dev, linear_dev, &cp, &pp, &ow_, &oh); st != OW_OK) return st;
    if (ow_status st = check_pixel_alignment(rgba8_dev, pixels_dev); st != OW_OK) return st;
    if ((uintptr_t)linear_dev & 15u) return fail(OW_ERR_INVALID, "linear_dev must be 16-byte aligned");
    OW_HIP(hipSetDevice(c->device));
    OW_HIP(ow::launch_present(ow_, oh, pp, (const ow::RenderPixel *)pixels_dev, (uint32_t *)rgba8_dev, linear_dev, main_stream(c)));
    return OW_OK;
}

}  // extern "C"

/* ---- light from the sky: the radiance pyramid and its pass (ow_sky_light.h, ow_sky_light.hip) ---- */

namespace {
void radiance_defaults(ow_radiance_options *o) {
    std::memset(o, 0, sizeof(*o));
    o->levels = ow::kRadianceDefaultLevels;
    o->samples = ow::kRadianceDefaultSamples;
    o->base_width = ow::kRadianceDefaultBase;
}
void radiance_light_defaults(ow_radiance_light_options *o) {
    std::memset(o, 0, sizeof(*o));
    o->ambient_energy = 1.0f;
    o->reflection_energy = 1.0f;
    o->specular = 0.5f;
}

// ow_radiance_options with the zeros resolved
ow_status resolve_radiance_options(const ow_radiance_options *opts, int *levels, int *samples, int *base_width) {
    static_assert(sizeof(ow_radiance_options) == sizeof(ow::RadianceOptions) && offsetof(ow_radiance_options, base_width) == offsetof(ow::RadianceOptions, base_width) &&
                      OW_RADIANCE_MAX_LEVELS == ow::kRadianceMaxLevels && OW_RADIANCE_MAX_SAMPLES == ow::kRadianceMaxSamples &&
                      OW_RADIANCE_IRRADIANCE == ow::kRadianceIrradiance,
                  "record layout");
    ow_radiance_options def;
    opts = or_defaults(opts, &def, radiance_defaults);
    *levels = opts->levels == 0 ? ow::kRadianceDefaultLevels : opts->levels;
    *samples = opts->samples == 0 ? ow::kRadianceDefaultSamples : opts->samples;
    *base_width = opts->base_width == 0 ? ow::kRadianceDefaultBase : opts->base_width;
    if (*levels < 2 || *levels > OW_RADIANCE_MAX_LEVELS) return fail(OW_ERR_INVALID, "ow_radiance_options: levels %d outside [2,%d]", opts->levels, OW_RADIANCE_MAX_LEVELS);
    if (*samples < 1 || *samples > OW_RADIANCE_MAX_SAMPLES)
        return fail(OW_ERR_INVALID, "ow_radiance_options: samples %d outside [1,%d]", opts->samples, OW_RADIANCE_MAX_SAMPLES);
    if (*base_width < ow::kRadianceMinBase || *base_width > ow::kRadianceMaxBase || (*base_width & (*base_width - 1)))
        return fail(OW_ERR_INVALID, "ow_radiance_options: base_width %d is not a power of two in [%d,%d]", opts->base_width, ow::kRadianceMinBase, ow::kRadianceMaxBase);
    return check_reserved(opts->reserved, "ow_radiance_options");
}

// ow_radiance_light_options (NULL = the defaults) -> the pass's constants; the pyramid's are filled in by radiance_light_apply
ow_status resolve_radiance_light_options(const ow_radiance_light_options *opts, ow::SkyLightParams *lp) {
    static_assert(sizeof(ow_radiance_light_options) == sizeof(ow::SkyLightOptions) &&
                      offsetof(ow_radiance_light_options, flags) == offsetof(ow::SkyLightOptions, flags) &&
                      offsetof(ow_radiance_light_options, reserved) == offsetof(ow::SkyLightOptions, reserved) && OW_RAY_SKY_LIT == ow::kRaySkyLit,
                  "record layout");
    ow_radiance_light_options def;
    opts = or_defaults(opts, &def, radiance_light_defaults);
    std::memset(lp, 0, sizeof(*lp));
    if (!in_range(opts->ambient_energy, 0.0f, ow::kSkyLightEnergyMax)) return fail(OW_ERR_INVALID, "ow_radiance_light_options: ambient_energy outside [0,1e12]");
    if (!in_range(opts->reflection_energy, 0.0f, ow::kSkyLightEnergyMax))
        return fail(OW_ERR_INVALID, "ow_radiance_light_options: reflection_energy outside [0,1e12]");
    if (!in_range(opts->specular, 0.0f, 1.0f)) return fail(OW_ERR_INVALID, "ow_radiance_light_options: specular outside [0,1]");
    if (opts->flags != 0u) return fail(OW_ERR_INVALID, "unknown radiance light flags 0x%x", opts->flags);
    if (ow_status st = check_reserved(opts->reserved, "ow_radiance_light_options"); st != OW_OK) return st;
    lp->ambient_energy = opts->ambient_energy;
    lp->reflection_energy = opts->reflection_energy;
    ow::sky_light_fresnel(opts->specular, lp->f0, lp->f50);
    lp->camera_ok = 1;
    return OW_OK;
}

// The pass in either form (pixel_pass).  The argument checks both forms share: ow_environment_apply's, in its order, then the context and the pyramid.
ow_status radiance_light_apply(ow_context *c, bool async, const ow_radiance *radiance, const ow_camera *camera, const ow_radiance_light_options *opts,
                               ow_render_pixel *pixels) {
    ow::CameraParams cp;
    ow::SkyLightParams lp;
    if (!pixels) return fail(OW_ERR_INVALID, "null argument: the records");
    if (ow_status st = resolve_camera(camera, &cp); st != OW_OK) return st;
    if (ow_status st = resolve_radiance_light_options(opts, &lp); st != OW_OK) return st;
    if (ow_status st = check_handle(c, radiance, "radiance pyramid"); st != OW_OK) return st;
    lp.levels = radiance->plan.levels;
    for (int k = 0; k < radiance->plan.levels; ++k) lp.R[k] = radiance->R[k];
    lp.E = radiance->E;
    lp.camera_ok = ow::mesh_camera_ok(cp) ? 1 : 0;
    return pixel_pass(c, async, (size_t)cp.width * cp.height, nullptr, pixels, [&](uint32_t *, ow::RenderPixel *pixels_dev) {
        OW_HIP(ow::launch_sky_light_apply(cp, lp, pixels_dev, main_stream(c)));
        return OW_OK;
    });
}
}  // namespace

extern "C" {

void ow_radiance_options_default(ow_radiance_options *out) {
    if (out) radiance_defaults(out);
}
void ow_radiance_light_options_default(ow_radiance_light_options *out) {
    if (out) radiance_light_defaults(out);
}

ow_status ow_radiance_create(ow_context *c, ow_sky *sky, const ow_radiance_options *opts, ow_radiance **out) {
    if (!out) return fail(OW_ERR_INVALID, "null argument");
    int levels, samples, base_width;
    if (ow_status st = resolve_radiance_options(opts, &levels, &samples, &base_width); st != OW_OK) return st;
    if (ow_status st = check_handle(c, sky, "sky"); st != OW_OK) return st;
    ow::RadianceBuild b;
    std::memset(&b, 0, sizeof(b));
    ow::RadiancePlan &p = b.plan;
    if (!ow::radiance_plan(sky->tex.width, sky->tex.height, levels, base_width, &p))
        return fail(OW_ERR_INVALID, "a %d x %d panorama has no %d exact levels at least 2 texels wide under base_width %d", sky->tex.width, sky->tex.height, levels,
                    base_width);
    p.samples = samples;
    // the block: R_0 (= M_0), R_1 .., M_1 .., E, then the host's tables in one piece (uploaded with one copy)
    constexpr size_t kTexel = 4 * sizeof(float);
    Layout L;
    size_t r_off[ow::kRadianceMaxLevels], m_off[ow::kRadianceMaxChain];
    for (int k = 0; k < levels; ++k) r_off[k] = L.take((size_t)p.width[k] * p.height[k] * kTexel);
    m_off[0] = r_off[0];
    for (int k = 1; k < p.chain; ++k) m_off[k] = L.take((size_t)p.width[k] * p.height[k] * kTexel);
    const size_t e_off = L.take((size_t)ow::kIrradianceWidth * ow::kIrradianceHeight * kTexel);
    std::vector<float> tables;
    const auto table = [&](size_t floats) {  // the offset, in floats, of a table; each starts 16-byte aligned
        const size_t at = tables.size();
        tables.resize(at + ((floats + 3) & ~(size_t)3));
        return at;
    };
    size_t col_at[ow::kRadianceMaxChain], row_at[ow::kRadianceMaxChain], smp_at[ow::kRadianceMaxLevels] = {};
    for (int k = 0; k < p.chain; ++k) {
        col_at[k] = table(2 * (size_t)p.width[k]);
        ow::radiance_dir_table(p.width[k], false, tables.data() + col_at[k]);
        row_at[k] = table(2 * (size_t)p.height[k]);
        ow::radiance_dir_table(p.height[k], true, tables.data() + row_at[k]);
    }
    for (int k = 1; k < levels; ++k) {
        smp_at[k] = table(4 * (size_t)samples);
        ow::radiance_sample_table((double)k / (double)(levels - 1), samples, tables.data() + smp_at[k]);
    }
    const size_t ecol_at = table(2 * ow::kIrradianceWidth), erow_at = table(2 * ow::kIrradianceHeight);
    ow::radiance_dir_table(ow::kIrradianceWidth, false, tables.data() + ecol_at);
    ow::radiance_dir_table(ow::kIrradianceHeight, true, tables.data() + erow_at);
    const size_t t_off = L.take(tables.size() * sizeof(float));
    ow_radiance *r;
    if (ow_status st = new_handle(c, L.total, "radiance pyramid", &r); st != OW_OK) return st;
    char *base = (char *)r->block;
    const float *tab = (const float *)(base + t_off);
    r->plan = p;
    for (int k = 0; k < levels; ++k) {
        b.R[k] = (float *)(base + r_off[k]);
        b.samples[k] = tab + smp_at[k];
        r->R[k] = ow::RadianceLevel{b.R[k], p.width[k], p.height[k]};
    }
    for (int k = 0; k < p.chain; ++k) {
        b.M[k] = (float *)(base + m_off[k]);
        b.col[k] = tab + col_at[k];
        b.row[k] = tab + row_at[k];
    }
    b.E = (float *)(base + e_off);
    b.ecol = tab + ecol_at;
    b.erow = tab + erow_at;
    r->E = ow::RadianceLevel{b.E, ow::kIrradianceWidth, ow::kIrradianceHeight};
    b.sky = sky->tex;
    b.srgb = sky->srgb;
    b.energy = sky->energy;
    // the sizes above level 0's live in a block of their own, freed behind the create's one synchronisation
    void *pre = nullptr;
    if (p.pre > 0) {
        Layout PL;
        size_t off[16];
        int w = sky->tex.width, h = sky->tex.height;
        for (int i = 0; i < p.pre; ++i, w /= 2, h /= 2) off[i] = PL.take((size_t)w * h * kTexel);
        if (hipMalloc(&pre, PL.total) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(r->block);
            delete r;
            return fail(OW_ERR_NOMEM, "hipMalloc failed for %zu bytes of radiance scratch", PL.total);
        }
        for (int i = 0; i < p.pre; ++i) b.pre[i] = (float *)((char *)pre + off[i]);
    }
    hipStream_t s = main_stream(c);
    const bool enqueued = hipMemcpyAsync(base + t_off, tables.data(), tables.size() * sizeof(float), hipMemcpyHostToDevice, s) == hipSuccess &&
                          ow::launch_radiance_build(b, s) == hipSuccess;
    const ow_status st = finish_create(c, r, s, enqueued, "radiance build", out);  // synchronises: `tables` and `pre` are done with
    if (pre) (void)hipFree(pre);
    return st;
}

void ow_radiance_destroy(ow_context *, ow_radiance *radiance) {
    if (radiance) release_handle(radiance);
    delete radiance;
}

ow_status ow_radiance_level(ow_context *c, ow_radiance *radiance, int32_t level, int32_t *levels, int32_t *width, int32_t *height, float *texels_out) {
    if (ow_status st = check_handle(c, radiance, "radiance pyramid"); st != OW_OK) return st;
    if (level != OW_RADIANCE_IRRADIANCE && (level < 0 || level >= radiance->plan.levels))
        return fail(OW_ERR_INVALID, "level %d outside [0,%d) and not OW_RADIANCE_IRRADIANCE", level, radiance->plan.levels);
    const ow::RadianceLevel &t = level == OW_RADIANCE_IRRADIANCE ? radiance->E : radiance->R[level];
    if (levels) *levels = radiance->plan.levels;
    if (width) *width = t.width;
    if (height) *height = t.height;
    if (!texels_out) return OW_OK;
    return read_back(c, texels_out, t.texels, (size_t)t.width * t.height * 4 * sizeof(float));
}

ow_status ow_radiance_light_apply(ow_context *c, ow_radiance *radiance, const ow_camera *camera, const ow_radiance_light_options *opts,
                                  ow_render_pixel *pixels_inout) {
    return radiance_light_apply(c, false, radiance, camera, opts, pixels_inout);
}

ow_status ow_radiance_light_apply_async(ow_context *c, ow_radiance *radiance, const ow_camera *camera, const ow_radiance_light_options *opts,
                                        ow_render_pixel *pixels_dev) {
    return radiance_light_apply(c, true, radiance, camera, opts, pixels_dev);
}

}  // extern "C"

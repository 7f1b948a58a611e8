// ow_spray_host.hip -- the sea spray: the ow_spray_* emitter over the kernels of ow_spray.hip (ow_spray.h), and its billboards, the
// ow_billboard_* materials and draws, over those of ow_spray_draw.hip (ow_spray_draw.h).
#include <cmath>
#include <cstring>

#include "ow_consumer_host.h"

using namespace ow::readside;
using ow::fail, ow::main_stream, ow::sync_stream;

extern "C" {

/* ---- the sea-spray emitter (ow_spray.h, ow_spray.hip) ---- */

void ow_spray_options_default(ow_spray_options *out) {
    static_assert(sizeof(ow_spray_options) == sizeof(ow::SprayOptions) && offsetof(ow_spray_options, particle_scale) == offsetof(ow::SprayOptions, particle_scale) &&
                      offsetof(ow_spray_options, emission_transform) == offsetof(ow::SprayOptions, emission_transform) &&
                      offsetof(ow_spray_options, start_time) == offsetof(ow::SprayOptions, start_time) &&
                      offsetof(ow_spray_options, reserved) == offsetof(ow::SprayOptions, reserved) &&
                      sizeof(ow_spray_instance) == sizeof(ow::SprayInstance) && offsetof(ow_spray_instance, custom) == offsetof(ow::SprayInstance, custom) &&
                      sizeof(ow_spray_particle) == sizeof(ow::SprayParticle) && offsetof(ow_spray_particle, particle_lifetime) == offsetof(ow::SprayParticle, particle_lifetime) &&
                      offsetof(ow_spray_particle, flags) == offsetof(ow::SprayParticle, flags) && OW_SPRAY_ACTIVE == ow::kSprayActive &&
                      OW_SPRAY_HAS_STARTED == ow::kSprayHasStarted && OW_SPRAY_RESTARTED == ow::kSprayRestarted &&
                      OW_SPRAY_MIN_AMOUNT == ow::kSprayMinAmount && OW_SPRAY_MAX_AMOUNT == ow::kSprayMaxAmount,
                  "record layout");
    if (!out) return;
    ow::spray_default_options((ow::SprayOptions *)out);
}

ow_status ow_spray_create(ow_context *c, const ow_spray_options *opts, ow_spray **out) {
    if (!opts || !out) return fail(OW_ERR_INVALID, "null argument");
    ow::SprayOptions o;
    std::memcpy(&o, opts, sizeof(o));
    ow::SprayParams P;
    ow::SprayHostState H;
    if (const char *why = ow::spray_resolve(o, &P, &H)) return fail(OW_ERR_INVALID, "ow_spray_options: %s", why);
    if (!c) return fail(OW_ERR_INVALID, "null context");
    const size_t amount = P.amount, blocks = (amount + ow::kSprayBlock - 1) / ow::kSprayBlock;
    Layout L;
    const size_t p_off = L.take(amount * sizeof(ow::SprayParticle)), i_off = L.take(amount * sizeof(ow::SprayInstance)), d_off = L.take(amount * sizeof(uint32_t));
    const size_t b_off = L.take(blocks * ow::kSprayBlockWords * sizeof(uint32_t));
    const size_t t_off = L.take(2 * sizeof(uint64_t) + sizeof(uint32_t));  // the two totals, the live count behind them
    ow_spray *e;
    if (ow_status st = new_handle(c, L.total, "particles", &e); st != OW_OK) return st;
    char *base = (char *)e->block;
    e->P = P;
    e->H = H;
    e->A.particles = (ow::SprayParticle *)(base + p_off);
    e->A.instances = (ow::SprayInstance *)(base + i_off);
    e->A.draw_list = (uint32_t *)(base + d_off);
    e->A.block_words = (uint32_t *)(base + b_off);
    e->A.totals = (uint64_t *)(base + t_off);
    e->A.live_count = (uint32_t *)(base + t_off + 2 * sizeof(uint64_t));
    hipStream_t s = main_stream(c);
    return finish_create(c, e, s, hipMemsetAsync(e->block, 0, L.total, s) == hipSuccess, "particle set-up", out);
}

void ow_spray_destroy(ow_context *, ow_spray *e) {
    if (e) release_handle(e);
    delete e;
}

ow_status ow_spray_step(ow_context *c, ow_spray *e, double delta, const float *map_scales, int32_t num_cascades) {
    if (!std::isfinite(delta) || !(delta > 0.0)) return fail(OW_ERR_INVALID, "delta must be finite and > 0");
    if (num_cascades < 1 || num_cascades > OW_MAX_CASCADES) return fail(OW_ERR_INVALID, "num_cascades %d outside [1,%d]", num_cascades, OW_MAX_CASCADES);
    if (!map_scales) return fail(OW_ERR_INVALID, "null argument");
    if (ow_status st = check_handle(c, e, "spray emitter"); st != OW_OK) return st;
    if (!ow::spray_delta_ok(e->P, delta)) return fail(OW_ERR_INVALID, "delta %g outside (0, emitter_lifetime = %g)", delta, (double)e->P.emitter_lifetime);
    if (ow_status st = check_point_query(c, 0, num_cascades); st != OW_OK) return st;
    if (ow_status st = begin_async(c, num_cascades); st != OW_OK) return st;
    ow::SprayHostState H = e->H;  // advanced only once the launches are in
    const ow::SprayClock K = ow::spray_advance(e->P, H, delta);
    const ow::MapsView v = view_of(c);
    OW_HIP(ow::launch_spray_step(v.n, num_cascades, v.buf, e->A, surface_scales(map_scales, num_cascades), e->P, K, v.stream));
    e->H = H;
    return OW_OK;
}

ow_status ow_spray_read(ow_context *c, ow_spray *e, ow_spray_instance *instances, ow_spray_particle *particles, uint32_t *draw_list, uint32_t *live_count) {
    if (ow_status st = check_handle(c, e, "spray emitter"); st != OW_OK) return st;
    OW_HIP(hipSetDevice(c->device));
    hipStream_t s = main_stream(c);
    uint32_t live = 0;
    if (instances) OW_HIP(hipMemcpyAsync(instances, e->A.instances, (size_t)e->P.amount * sizeof(ow::SprayInstance), hipMemcpyDeviceToHost, s));
    if (particles) OW_HIP(hipMemcpyAsync(particles, e->A.particles, (size_t)e->P.amount * sizeof(ow::SprayParticle), hipMemcpyDeviceToHost, s));
    OW_HIP(hipMemcpyAsync(&live, e->A.live_count, sizeof(live), hipMemcpyDeviceToHost, s));
    if (ow_status st = sync_stream(c, 0); st != OW_OK) return st;
    if (live > e->P.amount) return fail(OW_ERR_HIP, "live count %u beyond amount %u", live, e->P.amount);
    if (draw_list && live > 0) OW_HIP(hipMemcpy(draw_list, e->A.draw_list, (size_t)live * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (live_count) *live_count = live;
    return OW_OK;
}

ow_status ow_spray_get_device_ptrs(ow_context *c, ow_spray *e, void **instances, void **particles, void **draw_list, void **live_count) {
    if (ow_status st = check_handle(c, e, "spray emitter"); st != OW_OK) return st;
    if (instances) *instances = e->A.instances;
    if (particles) *particles = e->A.particles;
    if (draw_list) *draw_list = e->A.draw_list;
    if (live_count) *live_count = e->A.live_count;
    return OW_OK;
}

ow_status ow_spray_stats(ow_context *c, ow_spray *e, double *time, uint64_t *steps, uint64_t *restarts, uint64_t *spawned, uint64_t *rejected) {
    if (ow_status st = check_handle(c, e, "spray emitter"); st != OW_OK) return st;
    if (spawned || rejected) {
        uint64_t w[2] = {0, 0};
        if (ow_status st = read_back(c, w, e->A.totals, sizeof(w)); st != OW_OK) return st;
        if (spawned) *spawned = w[0];
        if (rejected) *rejected = w[1];
    }
    if (time) *time = e->H.time;
    if (steps) *steps = e->H.steps;
    if (restarts) *restarts = e->H.restarts;
    return OW_OK;
}

}  // extern "C"

/* ---- the spray billboards (ow_spray_draw.h, ow_spray_draw.hip) ---- */

namespace {
constexpr size_t kBillboardHead = 16;                    // the two counters (and two words of padding) ahead of the masks

// where a draw's arrays lie in the context's scratch block
struct BillboardPlan {
    ow::BillboardBins bins;
    size_t sprites_off, instances_off, total;
};
BillboardPlan billboard_plan(int width, int height, uint32_t slots, int bin_side, bool upload) {
    BillboardPlan p;
    p.bins = ow::billboard_bins(width, height, slots, bin_side);
    Layout L;
    L.take(kBillboardHead + (size_t)p.bins.nx * p.bins.ny * p.bins.words * sizeof(uint64_t));  // the counters and the masks, at 0
    p.sprites_off = L.take((size_t)slots * sizeof(ow::SpraySprite));
    p.instances_off = L.take(upload ? (size_t)slots * sizeof(ow::SprayInstance) : 0);
    p.total = L.total;
    return p;
}

// ow_billboard_draw_options (NULL = the defaults) -> the draw's own constants
ow_status resolve_billboard_options(const ow_billboard_draw_options *o, ow::SprayDrawParams *dp, int *bin_side) {
    static_assert(sizeof(ow_billboard_draw_options) == sizeof(ow::BillboardDrawOptions) && offsetof(ow_billboard_draw_options, bin_side) == offsetof(ow::BillboardDrawOptions, bin_side) &&
                      sizeof(ow_billboard_material_options) == sizeof(ow::BillboardMaterialOptions) &&
                      offsetof(ow_billboard_material_options, albedo_srgb) == offsetof(ow::BillboardMaterialOptions, albedo_srgb) &&
                      OW_BILLBOARD_TEXTURE_MAX_SIDE == ow::kBillboardTexMaxSide,
                  "record layout");
    dp->near = ow::kMeshDefaultNear;
    dp->background[0] = dp->background[1] = dp->background[2] = 0.0f;
    *bin_side = ow::kBillboardBinSide;
    if (!o) return OW_OK;
    if (!std::isfinite(o->near)) return fail(OW_ERR_INVALID, "near is not finite");
    for (float v : o->background_color)
        if (!std::isfinite(v)) return fail(OW_ERR_INVALID, "background_color is not finite");
    if (o->bin_side != 0 && (o->bin_side < 8 || o->bin_side > ow::kBillboardBinMax || o->bin_side % 8 != 0))
        return fail(OW_ERR_INVALID, "bin_side %d is not 0 or a multiple of 8 in [8,%d]", o->bin_side, ow::kBillboardBinMax);
    if (o->flags != 0u) return fail(OW_ERR_INVALID, "unknown billboard flags 0x%x", o->flags);
    if (ow_status st = check_reserved(o->reserved, "ow_billboard_draw_options"); st != OW_OK) return st;
    if (o->near > 0.0f) dp->near = o->near;
    for (int k = 0; k < 3; ++k) dp->background[k] = o->background_color[k];
    if (o->bin_side > 0) *bin_side = o->bin_side;
    return OW_OK;
}

// the argument checks every form of the draw shares: ow_mesh_draw's, in its order, then the context and the material
ow_status check_billboard_draw(const ow_context *c, const ow_billboard_material *m, const ow_camera *camera, const ow_billboard_draw_options *opts,
                               const void *pixels, const void *rgba, ow::CameraParams *cp, ow::SprayDrawParams *dp, int *bin_side) {
    if (!rgba && !pixels) return fail(OW_ERR_INVALID, "null argument: both outputs");
    if (ow_status st = resolve_camera(camera, cp); st != OW_OK) return st;
    if (ow_status st = resolve_billboard_options(opts, dp, bin_side); st != OW_OK) return st;
    if (ow_status st = check_handle(c, m, "billboard material"); st != OW_OK) return st;
    dp->camera_ok = ow::mesh_camera_ok(*cp) ? 1 : 0;
    for (int k = 0; k < 3; ++k) dp->foam[k] = m->foam[k];
    dp->max_alpha = m->max_alpha;
    dp->albedo = m->albedo;
    dp->dissolve = m->dissolve;
    dp->srgb = m->srgb;
    dp->time = 0.0f;
    return OW_OK;
}

// The scratch of a draw and its launches on the context's stream.  Sources: an emitter's resident arrays, or `upload` (host instances, copied
// into the scratch first).  A block that has to grow while launches already enqueued may still read it is replaced behind one synchronisation
// (sync_before_growth).
ow_status billboard_enqueue(ow_context *c, const ow::CameraParams &cp, const ow::SprayDrawParams &dp, int bin_side, const ow_spray *e,
                            const ow_spray_instance *upload, uint32_t slots, ow::RenderPixel *pixels_dev, uint32_t *rgba_dev) {
    const BillboardPlan p = billboard_plan(cp.width, cp.height, slots, bin_side, upload != nullptr);
    if (ow_status st = sync_before_growth(c, c->billboard, p.total); st != OW_OK) return st;
    if (ow_status st = c->billboard.ensure(p.total, 0, 1, "bytes of billboard scratch"); st != OW_OK) return st;
    char *base = (char *)c->billboard.ptr;
    hipStream_t s = main_stream(c);
    ow::BillboardArrays A;
    A.slots = slots;
    A.counters = (uint32_t *)base;
    A.masks = (uint64_t *)(base + kBillboardHead);
    A.clear_bytes = kBillboardHead + (size_t)p.bins.nx * p.bins.ny * p.bins.words * sizeof(uint64_t);
    A.sprites = (ow::SpraySprite *)(base + p.sprites_off);
    if (e) {
        A.instances = e->A.instances;
        A.draw_list = e->A.draw_list;
        A.live_count = e->A.live_count;
    } else {
        A.instances = (const ow::SprayInstance *)(base + p.instances_off);
        A.draw_list = nullptr;
        A.live_count = nullptr;
        if (slots > 0) OW_HIP(hipMemcpyAsync(base + p.instances_off, upload, (size_t)slots * sizeof(ow::SprayInstance), hipMemcpyHostToDevice, s));
    }
    OW_HIP(ow::launch_billboard_draw(A, cp, dp, p.bins, rgba_dev, pixels_dev, s));
    ++c->billboard_draws;
    return OW_OK;
}

// a draw in either form (pixel_pass) over the caller's records
ow_status billboard_draw(ow_context *c, bool async, const ow::CameraParams &cp, const ow::SprayDrawParams &dp, int bin_side, const ow_spray *e,
                         const ow_spray_instance *upload, uint32_t slots, ow_render_pixel *pixels, void *rgba8) {
    return pixel_pass(c, async, (size_t)cp.width * cp.height, rgba8, pixels, [&](uint32_t *rgba_dev, ow::RenderPixel *pixels_dev) {
        return billboard_enqueue(c, cp, dp, bin_side, e, upload, slots, pixels_dev, rgba_dev);
    });
}
}  // namespace

extern "C" {

void ow_billboard_material_options_default(ow_billboard_material_options *out) {
    if (!out) return;
    ow_render_options ro;
    render_defaults(&ro);
    std::memset(out, 0, sizeof(*out));
    for (int k = 0; k < 3; ++k) out->foam_color[k] = ro.foam_color[k];
    out->max_alpha = ow::kBillboardMaxAlpha;
    out->albedo_srgb = out->dissolve_srgb = 1u;
}

ow_status ow_billboard_material_create(ow_context *c, const ow_billboard_material_options *opts, const void *albedo_rgba8, int32_t albedo_width,
                                       int32_t albedo_height, const void *dissolve_rgba8, int32_t dissolve_width, int32_t dissolve_height,
                                       ow_billboard_material **out) {
    if (!opts || !out) return fail(OW_ERR_INVALID, "null argument");
    for (float v : opts->foam_color)
        if (!(std::fabs(v) <= 1e38f)) return fail(OW_ERR_INVALID, "ow_billboard_material_options: foam_color is not finite (or beyond 1e38)");
    if (!(opts->max_alpha >= 0.0f && opts->max_alpha <= 1.0f)) return fail(OW_ERR_INVALID, "ow_billboard_material_options: max_alpha outside [0,1]");
    if (opts->albedo_srgb > 1u || opts->dissolve_srgb > 1u) return fail(OW_ERR_INVALID, "ow_billboard_material_options: an sRGB flag is not 0 or 1");
    if (ow_status st = check_reserved(opts->reserved, "ow_billboard_material_options"); st != OW_OK) return st;
    const int32_t sides[4] = {albedo_width, albedo_height, dissolve_width, dissolve_height};
    for (int32_t v : sides)
        if (v < 1 || v > OW_BILLBOARD_TEXTURE_MAX_SIDE) return fail(OW_ERR_INVALID, "texture side %d outside [1,%d]", v, OW_BILLBOARD_TEXTURE_MAX_SIDE);
    if (!albedo_rgba8 || !dissolve_rgba8) return fail(OW_ERR_INVALID, "null argument");
    if (!c) return fail(OW_ERR_INVALID, "null context");
    float table[256];
    ow::spray_srgb_table(table);
    const size_t a_bytes = (size_t)albedo_width * albedo_height * 4, d_bytes = (size_t)dissolve_width * dissolve_height * 4;
    Layout L;
    const size_t t_off = L.take(sizeof(table)), a_off = L.take(a_bytes), d_off = L.take(d_bytes);
    ow_billboard_material *m;
    if (ow_status st = new_handle(c, L.total, "textures", &m); st != OW_OK) return st;
    char *base = (char *)m->block;
    m->srgb = (const float *)(base + t_off);
    m->albedo = ow::SprayTexture{(const uint32_t *)(base + a_off), albedo_width, albedo_height, (int)opts->albedo_srgb};
    m->dissolve = ow::SprayTexture{(const uint32_t *)(base + d_off), dissolve_width, dissolve_height, (int)opts->dissolve_srgb};
    for (int k = 0; k < 3; ++k) m->foam[k] = opts->foam_color[k];
    m->max_alpha = opts->max_alpha;
    hipStream_t s = main_stream(c);
    const bool enqueued = hipMemcpyAsync((void *)m->srgb, table, sizeof(table), hipMemcpyHostToDevice, s) == hipSuccess &&
                          hipMemcpyAsync((void *)m->albedo.texels, albedo_rgba8, a_bytes, hipMemcpyHostToDevice, s) == hipSuccess &&
                          hipMemcpyAsync((void *)m->dissolve.texels, dissolve_rgba8, d_bytes, hipMemcpyHostToDevice, s) == hipSuccess;
    return finish_create(c, m, s, enqueued, "texture upload", out);
}

void ow_billboard_material_destroy(ow_context *, ow_billboard_material *m) {
    if (m) release_handle(m);
    delete m;
}

ow_status ow_billboard_draw(ow_context *c, ow_spray *e, ow_billboard_material *m, const ow_camera *camera, const ow_billboard_draw_options *opts,
                            ow_render_pixel *pixels_inout, void *rgba8_out) {
    ow::CameraParams cp;
    ow::SprayDrawParams dp;
    int bin_side;
    if (ow_status st = check_billboard_draw(c, m, camera, opts, pixels_inout, rgba8_out, &cp, &dp, &bin_side); st != OW_OK) return st;
    if (ow_status st = check_handle(c, e, "spray emitter"); st != OW_OK) return st;
    dp.time = (float)e->H.time;
    return billboard_draw(c, false, cp, dp, bin_side, e, nullptr, e->P.amount, pixels_inout, rgba8_out);
}

ow_status ow_billboard_draw_async(ow_context *c, ow_spray *e, ow_billboard_material *m, const ow_camera *camera, const ow_billboard_draw_options *opts,
                                  ow_render_pixel *pixels_dev, void *rgba8_dev) {
    ow::CameraParams cp;
    ow::SprayDrawParams dp;
    int bin_side;
    if (ow_status st = check_billboard_draw(c, m, camera, opts, pixels_dev, rgba8_dev, &cp, &dp, &bin_side); st != OW_OK) return st;
    if (ow_status st = check_handle(c, e, "spray emitter"); st != OW_OK) return st;
    dp.time = (float)e->H.time;
    return billboard_draw(c, true, cp, dp, bin_side, e, nullptr, e->P.amount, pixels_dev, rgba8_dev);
}

ow_status ow_billboard_draw_instances(ow_context *c, ow_billboard_material *m, const ow_spray_instance *instances, int32_t count, float time,
                                      const ow_camera *camera, const ow_billboard_draw_options *opts, ow_render_pixel *pixels_inout, void *rgba8_out) {
    if (count < 0 || (uint32_t)count > OW_SPRAY_MAX_AMOUNT) return fail(OW_ERR_INVALID, "count %d outside [0,%u]", count, OW_SPRAY_MAX_AMOUNT);
    if (count > 0 && !instances) return fail(OW_ERR_INVALID, "null argument");
    if (!std::isfinite(time)) return fail(OW_ERR_INVALID, "time is not finite");
    ow::CameraParams cp;
    ow::SprayDrawParams dp;
    int bin_side;
    if (ow_status st = check_billboard_draw(c, m, camera, opts, pixels_inout, rgba8_out, &cp, &dp, &bin_side); st != OW_OK) return st;
    dp.time = time;
    return billboard_draw(c, false, cp, dp, bin_side, nullptr, instances, (uint32_t)count, pixels_inout, rgba8_out);
}

ow_status ow_billboard_draw_stats(ow_context *c, uint64_t *draws, uint64_t *culled, uint64_t *drawn, uint64_t *scratch_bytes) {
    if (!c) return fail(OW_ERR_INVALID, "null context");
    if (culled || drawn) {
        uint32_t w[2] = {0, 0};
        if (c->billboard.ptr)  // no draw yet: zeros, and the device is not touched
            if (ow_status st = read_back(c, w, c->billboard.ptr, sizeof(w)); st != OW_OK) return st;
        if (drawn) *drawn = w[0];
        if (culled) *culled = w[1];
    }
    if (draws) *draws = c->billboard_draws;
    if (scratch_bytes) *scratch_bytes = c->billboard.bytes;
    return OW_OK;
}

}  // extern "C"

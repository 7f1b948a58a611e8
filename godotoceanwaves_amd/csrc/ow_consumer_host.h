// ow_consumer_host.h -- what the host units of the read side share (ow_consumer_host.hip and the ow_*_host.hip beside it; nobody else
// includes this).  A name is here because more than one subsystem uses it; what one subsystem uses alone stays in its unit's anonymous namespace.
// Templates are defined here, everything else once in the unit named beside it (no name: ow_consumer_host.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <new>

#include "ow_context.h"

namespace ow::readside {
// ---- the context and the argument checks ----
// the context's own maps, for an enqueue behind everything on its stream (main_stream(): behind the second chain's join as well)
MapsView view_of(ow_context *c);
// what every asynchronous form does between its argument checks and its first enqueue
ow_status begin_async(ow_context *c, int num_cascades);
// the first num_cascades map_scales records as a launch takes them
SurfaceScales surface_scales(const float *map_scales, int num_cascades);
// the argument checks ow_sample_surface makes, shared by every call that takes num_cascades (count == 0 is fine and does nothing)
ow_status check_point_query(const ow_context *c, int32_t count, int32_t num_cascades);
// ... and what both forms of a call over `count` points or rays check before they touch the device; count == 0 passes (the caller returns OW_OK)
template <class Options, class Params>
ow_status check_point_call(const ow_context *c, const void *in, int32_t count, const float *map_scales, int32_t num_cascades, const Options *opts,
                           ow_status (*resolve)(const Options *, Params *), Params *params, const void *out) {
    if (ow_status st = check_point_query(c, count, num_cascades); st != OW_OK) return st;
    if (ow_status st = resolve(opts, params); st != OW_OK) return st;
    if (count > 0 && (!in || !map_scales || !out)) return fail(OW_ERR_INVALID, "null argument");
    return OW_OK;
}

// an option struct's reserved words (`name`: the struct's)
template <size_t N>
ow_status check_reserved(const uint32_t (&reserved)[N], const char *name) {
    for (uint32_t r : reserved)
        if (r != 0u) return fail(OW_ERR_INVALID, "%s.reserved must be 0", name);
    return OW_OK;
}
// lo <= v <= hi; false for a NaN
bool in_range(float v, float lo, float hi);
// an options record's lane_box, checked, and as a set-up reads it (ow_mesh.h mesh_lane_box; out may be null: ow_shadow.h shadow_params maps its own)
ow_status resolve_lane_box(int32_t lane_box, int *out);
// `opts`, or `def` filled in by `defaults` where the caller passed NULL
template <class Options>
const Options *or_defaults(const Options *opts, Options *def, void (*defaults)(Options *)) {
    if (opts) return opts;
    defaults(def);
    return def;
}

// ---- the handles' one life cycle (ow_context.h ow::Handle): Layout places a block's arrays, new_handle allocates, finish_create
// synchronises and registers, release_handle is the device half of a destroy ----
// a handle (`what`: a body set, a mesh) that belongs to this context
ow_status check_handle(const ow_context *c, const Handle *h, const char *what);
// The device half of a destroy; the caller deletes its own type.  An orphan (ow_destroy cleared ctx and freed the block) has none.
void release_handle(Handle *h);
// Where the arrays of one device block lie: each starts 256-byte aligned, in the order they are taken.
struct Layout {
    size_t total = 0;
    size_t take(size_t bytes) {  // the offset of the next array of `bytes`
        const size_t off = total;
        total += (bytes + 255) & ~(size_t)255;
        return off;
    }
};

// A handle of c with a block of `total` bytes of `what` on c's device (made current).  On failure there is no handle.
template <class H>
ow_status new_handle(ow_context *c, size_t total, const char *what, H **out) {
    OW_HIP(hipSetDevice(c->device));
    H *h = new (std::nothrow) H();
    if (!h) return fail(OW_ERR_NOMEM, "out of host memory");
    if (hipMalloc(&h->block, total) != hipSuccess) {
        (void)hipGetLastError();
        delete h;
        return fail(OW_ERR_NOMEM, "hipMalloc failed for %zu bytes of %s", total, what);
    }
    h->ctx = c;
    *out = h;
    return OW_OK;
}
// The end of a create whose set-up went onto stream s (`enqueued`: all of it did): one counted synchronisation, then the handle is on the
// context's list and the caller's.  On failure "<what> failed: <the HIP error>", and the handle and its block are gone.
template <class H>
ow_status finish_create(ow_context *c, H *h, hipStream_t s, bool enqueued, const char *what, H **out) {
    if (!enqueued || (++c->host_syncs, hipStreamSynchronize(s)) != hipSuccess) {
        const ow_status st = fail(OW_ERR_HIP, "%s failed: %s", what, hipGetErrorString(hipGetLastError()));
        (void)hipFree(h->block);
        delete h;
        return st;
    }
    c->handles.push_back(h);
    *out = h;
    return OW_OK;
}

// ---- readback ----
// a synchronising read of device memory: everything the context has enqueued has finished, and has not faulted, first
ow_status read_back(ow_context *c, void *dst, const void *src, size_t bytes);
constexpr size_t kCounterHead = 256;  // the four class counters, at the head of the solid draw's scratch and of a shadow map's block
// the four counters of a mesh draw, a solid draw or a shadow map into n[kTriSkipped .. kTriWave]; zeros where nothing is `wanted` or there are none yet
ow_status read_class_counts(ow_context *c, const void *counters_dev, bool wanted, uint64_t n[4]);

// ---- pictures ----
// ow_camera -> the kernel's camera; OW_ERR_INVALID for a size out of range or reserved words.  Non-finite values pass: they make every ray invalid.
ow_status resolve_camera(const ow_camera *cam, CameraParams *cp);
// an asynchronous form's output pointers (either may be null)
ow_status check_pixel_alignment(const void *rgba8_dev, const void *pixels_dev);
// one counted synchronisation where a scratch block that launches already enqueued may still read has to grow to `need` bytes
ow_status sync_before_growth(ow_context *c, const DeviceScratch &scratch, size_t need);
// Every synchronous picture call (views, mesh draws, billboard draws, solid draws), on the context's device: `enqueue(rgba_dev, pixels_dev)` writes `count`
// RGBA8 words and / or records into the context's pixel blocks (exact size; a null output's pointer is null), what was asked for is copied to
// the host behind it, and the stream is synchronised for the layers of `mask`.  upload_records: the records go up first (the billboards blend
// over them, the solids are tested against them).
template <class Enqueue>
ow_status picture_round_trip(ow_context *c, size_t count, void *rgba8_out, ow_render_pixel *pixels_out, bool upload_records, uint32_t mask, Enqueue enqueue) {
    if (rgba8_out)
        if (ow_status st = c->render_rgba.ensure(count * sizeof(uint32_t), 0, sizeof(uint32_t), "pixels"); st != OW_OK) return st;
    if (pixels_out)
        if (ow_status st = c->render_pixels.ensure(count * sizeof(ow::RenderPixel), 0, sizeof(ow::RenderPixel), "pixel records"); st != OW_OK) return st;
    uint32_t *rgba_dev = rgba8_out ? (uint32_t *)c->render_rgba.ptr : nullptr;
    ow::RenderPixel *pixels_dev = pixels_out ? (ow::RenderPixel *)c->render_pixels.ptr : nullptr;
    if (upload_records && pixels_out) OW_HIP(hipMemcpyAsync(pixels_dev, pixels_out, count * sizeof(ow::RenderPixel), hipMemcpyHostToDevice, main_stream(c)));
    if (ow_status st = enqueue(rgba_dev, pixels_dev); st != OW_OK) return st;
    if (rgba8_out) OW_HIP(hipMemcpyAsync(rgba8_out, rgba_dev, count * sizeof(uint32_t), hipMemcpyDeviceToHost, main_stream(c)));
    if (pixels_out) OW_HIP(hipMemcpyAsync(pixels_out, pixels_dev, count * sizeof(ow::RenderPixel), hipMemcpyDeviceToHost, main_stream(c)));
    return sync_stream(c, mask);
}
// A call that works on `count` records the caller already has (the in-place pixel passes; the billboard and solid draws), in either form, on
// the context's device.  The synchronous form is picture_round_trip with the records uploaded first and no layer to refuse (nothing here
// reads a map); the asynchronous form checks the caller's device pointers and enqueues on them.  `launch(rgba_dev, pixels_dev)` is the one launch.
template <class Launch>
ow_status pixel_pass(ow_context *c, bool async, size_t count, void *rgba8, ow_render_pixel *pixels, Launch launch) {
    if (async)
        if (ow_status st = check_pixel_alignment(rgba8, pixels); st != OW_OK) return st;
    OW_HIP(hipSetDevice(c->device));
    if (async) return launch((uint32_t *)rgba8, (RenderPixel *)pixels);
    return picture_round_trip(c, count, rgba8, pixels, true, 0, launch);
}

// ---- what one subsystem lends another ----
// the reference scene's material and sun (ow_render_options_default); the mesh, the billboards, the solids, the environment and the shadow
// frame take their defaults from it (ow_points_host.hip)
void render_defaults(ow_render_options *o);
// ow_render_options (NULL = the defaults) -> the hit's settings and the shading's; the mesh's material goes through it (ow_points_host.hip)
ow_status resolve_render_options(const ow_render_options *opts, RaycastParams *rp, ShadeParams *sp);
// the per-cascade bound words of the slab on the current device, allocated by the first ray cast or view that needs them (ow_points_host.hip)
ow_status ray_bound_words(uint32_t **bound);
// the stale layers of `mask` recomputed in stream order; point queries and buoyancy read them (ow_points_host.hip)
ow_status velocity_refresh(ow_context *c, uint32_t mask);
// Where the instances of a solid draw or a shadow cast come from: a body set's resident pose records and fault flags, or `upload` (host
// transforms: instance_upload_bytes of the caller's scratch at `staging`, copied there on `s` first), and their checks (ow_solid_host.hip)
size_t instance_upload_bytes(const float *upload, int count);
ow_status instance_source(const ow_bodies *set, int first, const float *upload, int count, void *staging, hipStream_t s, SolidInstances *in);
ow_status check_solid_count(const ow_solid *solid, int64_t count);
ow_status check_solid_bodies(const ow_context *c, const ow_solid *solid, const ow_bodies *set, int32_t first, int32_t count);
}  // namespace ow::readside

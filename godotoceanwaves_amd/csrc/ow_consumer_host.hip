// ow_consumer_host.hip -- what the read side's host units share (ow_consumer_host.h): the grow-only device scratch, the context and
// argument checks, the handles' life cycle, the camera and the picture calls' synchronisation rule, readback.  The entry points of
// include/ocean_waves.h are in the ow_*_host.hip beside it, one unit per subsystem.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "ow_consumer_host.h"

namespace ow {
ow_status DeviceScratch::ensure(size_t need, size_t floor, size_t unit, const char *what) {
    if (need <= bytes) return OW_OK;
    release();
    const size_t cap = std::max(need, floor);
    if (hipMalloc(&ptr, cap) != hipSuccess) {
        ptr = nullptr;
        return fail(OW_ERR_NOMEM, "hipMalloc failed for %zu %s", cap / unit, what);
    }
    bytes = cap;
    return OW_OK;
}
void DeviceScratch::release() {
    (void)hipFree(ptr);
    ptr = nullptr;
    bytes = 0;
}
}  // namespace ow

namespace ow::readside {
// the context's own maps, for an enqueue behind everything on its stream (main_stream(): behind the second chain's join as well)
ow::MapsView view_of(ow_context *c) { return ow::MapsView{c->n, c->buf, main_stream(c), c->device}; }

// the argument checks ow_sample_surface makes, shared by every call that takes num_cascades (count == 0 is fine and does nothing)
ow_status check_point_query(const ow_context *c, int32_t count, int32_t num_cascades) {
    if (!c) return fail(OW_ERR_INVALID, "null context");
    if (count < 0) return fail(OW_ERR_INVALID, "count must be >= 0");
    if (num_cascades < 1 || num_cascades > c->cascades) return fail(OW_ERR_INVALID, "num_cascades %d outside [1,%d]", num_cascades, c->cascades);
    return OW_OK;
}

// a synchronising read of device memory: everything the context has enqueued has finished, and has not faulted, first
ow_status read_back(ow_context *c, void *dst, const void *src, size_t bytes) {
    OW_HIP(hipSetDevice(c->device));
    if (ow_status st = sync_stream(c, 0); st != OW_OK) return st;
    if (bytes > 0) OW_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return OW_OK;
}

// The four counters of a mesh draw, a solid draw or a shadow map read back into n[kTriSkipped .. kTriWave] (kSolid* and kShadow* are defined
// as these): skipped (triangles of a mesh, instances of a solid or a cast), culled, and the two drawn classes.  Zeros, and the device is not
// touched, where nothing is `wanted` or there are no counters yet.
ow_status read_class_counts(ow_context *c, const void *counters_dev, bool wanted, uint64_t n[4]) {
    uint32_t w[4] = {0, 0, 0, 0};
    if (wanted && counters_dev)
        if (ow_status st = read_back(c, w, counters_dev, sizeof(w)); st != OW_OK) return st;
    for (int k = 0; k < 4; ++k) n[k] = w[k];
    return OW_OK;
}
// an options record's lane_box, checked, and as a set-up reads it (ow_mesh.h mesh_lane_box; out may be null: ow_shadow.h shadow_params maps its own)
ow_status resolve_lane_box(int32_t lane_box, int *out) {
    if (lane_box < -1 || lane_box > 64) return fail(OW_ERR_INVALID, "lane_box %d outside [-1,64]", lane_box);
    if (out) *out = ow::mesh_lane_box(lane_box);
    return OW_OK;
}

ow::SurfaceScales surface_scales(const float *map_scales, int num_cascades) {
    ow::SurfaceScales sc;
    std::memset(&sc, 0, sizeof(sc));
    std::memcpy(sc.s, map_scales, (size_t)num_cascades * 4 * sizeof(float));
    return sc;
}

// what every asynchronous form does between its argument checks and its first enqueue
ow_status begin_async(ow_context *c, int num_cascades) {
    if (ow_status st = refuse_faulted(c, layer_mask(num_cascades)); st != OW_OK) return st;
    OW_HIP(hipSetDevice(c->device));
    return OW_OK;
}

// ---- the handles' one life cycle (ow_context.h ow::Handle) ------------------------------------------------------------------------------
// a handle (`what`: a body set, a mesh) that belongs to this context
ow_status check_handle(const ow_context *c, const ow::Handle *h, const char *what) {
    if (!c) return fail(OW_ERR_INVALID, "null context");
    if (!h) return fail(OW_ERR_INVALID, "null %s", what);
    if (!h->ctx) return fail(OW_ERR_STATE, "the %s's context has been destroyed", what);
    if (h->ctx != c) return fail(OW_ERR_INVALID, "the %s belongs to another context", what);
    return OW_OK;
}
// The device half of a destroy; the caller deletes its own type.  An orphan (ow_destroy cleared ctx and freed the block) has none.
void release_handle(ow::Handle *h) {
    ow_context *c = h->ctx;
    if (!c) return;
    (void)hipSetDevice(c->device);
    ++c->host_syncs;
    (void)hipStreamSynchronize(main_stream(c));
    c->handles.erase(std::remove(c->handles.begin(), c->handles.end(), h), c->handles.end());
    (void)hipFree(h->block);
}

// ow_camera -> the kernel's camera; OW_ERR_INVALID for a size out of range or reserved words.  Non-finite values pass: they make every ray invalid.
ow_status resolve_camera(const ow_camera *cam, ow::CameraParams *cp) {
    if (!cam) return fail(OW_ERR_INVALID, "null camera");
    if (cam->width < 1 || cam->width > OW_RENDER_MAX_SIDE || cam->height < 1 || cam->height > OW_RENDER_MAX_SIDE)
        return fail(OW_ERR_INVALID, "camera size %d x %d outside [1,%d]", cam->width, cam->height, OW_RENDER_MAX_SIDE);
    if (ow_status st = check_reserved(cam->reserved, "ow_camera"); st != OW_OK) return st;
    for (int k = 0; k < 3; ++k) cp->o[k] = cam->position[k];
    for (int k = 0; k < 9; ++k) cp->B[k] = cam->basis[k];
    cp->tan_half_fov = (float)std::tan((double)cam->fov_y_degrees * (3.14159265358979323846 / 360.0));
    cp->aspect = (float)cam->width / (float)cam->height;
    cp->max_distance = cam->max_distance;
    cp->width = cam->width;
    cp->height = cam->height;
    return OW_OK;
}
ow_status check_pixel_alignment(const void *rgba8_dev, const void *pixels_dev) {
    if (((uintptr_t)rgba8_dev & 3u) || ((uintptr_t)pixels_dev & 15u)) return fail(OW_ERR_INVALID, "rgba8_dev must be 4-byte and pixels_dev 16-byte aligned");
    return OW_OK;
}
// Launches already enqueued (the asynchronous forms) may still read a scratch block that exists and has to grow to `need` bytes: one counted
// synchronisation through main_stream before DeviceScratch::ensure replaces it.
ow_status sync_before_growth(ow_context *c, const ow::DeviceScratch &scratch, size_t need) {
    if (scratch.ptr && need > scratch.bytes) {
        ++c->host_syncs;
        OW_HIP(hipStreamSynchronize(main_stream(c)));
    }
    return OW_OK;
}
bool in_range(float v, float lo, float hi) { return v >= lo && v <= hi; }  // false for a NaN
}  // namespace ow::readside

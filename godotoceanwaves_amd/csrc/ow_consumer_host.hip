// ow_consumer_host.hip -- the read side of include/ocean_waves.h: host wrappers around the kernels of ow_consumer.hip, ow_velocity.hip,
// ow_mesh.hip, ow_spray.hip, ow_spray_draw.hip, ow_solid.hip, ow_environment.hip, ow_sky_light.hip and ow_shadow.hip (surface samples and queries, buoyancy, floating bodies, ray casts, camera views, mesh draws,
// the velocity layers, the sea-spray emitter and its billboards, the solids, the environment pass, the present, the radiance pyramid and its pass, the sun shadows).  Plain C++ over
// the HIP runtime API; the context and the scheduler's services come from ow_context.h.  The synchronous calls' device halves (ow_internal.h
// *_round_trip) also serve a group's gathered arrays (ow_group.hip).
//
// Each repeated thing has one owner here.  The eight handle kinds (body sets, meshes, emitters, billboard materials, solid shapes, skies, radiance pyramids, shadow maps) share one life cycle:
// Layout places a block's arrays, new_handle allocates, finish_create synchronises and registers, release_handle is the device half of a
// destroy, check_handle the one ownership check.  The four picture kinds (views, mesh draws, billboard draws, solid draws) keep their launch in one
// *_enqueue each, used by the asynchronous form directly and by the synchronous form through picture_round_trip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <new>
#include <vector>

#include "ow_context.h"

namespace {
using ow::check_cascade, ow::fail, ow::layer_mask, ow::main_stream, ow::plane, ow::refuse_faulted, ow::sync_stream;

// the context's own maps, for an enqueue behind everything on its stream (main_stream(): behind the second chain's join as well)
ow::MapsView view_of(ow_context *c) { return ow::MapsView{c->n, c->buf, main_stream(c), c->device}; }

// the argument checks ow_sample_surface makes, shared by every call that takes num_cascades (count == 0 is fine and does nothing)
ow_status check_point_query(const ow_context *c, int32_t count, int32_t num_cascades) {
    if (!c) return fail(OW_ERR_INVALID, "null context");
    if (count < 0) return fail(OW_ERR_INVALID, "count must be >= 0");
    if (num_cascades < 1 || num_cascades > c->cascades) return fail(OW_ERR_INVALID, "num_cascades %d outside [1,%d]", num_cascades, c->cascades);
    return OW_OK;
}
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

// Where the arrays of one device block lie: each starts 256-byte aligned, in the order they are taken.
struct Layout {
    size_t total = 0;
    size_t take(size_t bytes) {  // the offset of the next array of `bytes`
        const size_t off = total;
        total += (bytes + 255) & ~(size_t)255;
        return off;
    }
};

// a synchronising read of device memory: everything the context has enqueued has finished, and has not faulted, first
ow_status read_back(ow_context *c, void *dst, const void *src, size_t bytes) {
    OW_HIP(hipSetDevice(c->device));
    if (ow_status st = sync_stream(c, 0); st != OW_OK) return st;
    if (bytes > 0) OW_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return OW_OK;
}

constexpr size_t kCounterHead = 256;  // the four class counters, at the head of the solid draw's scratch and of a shadow map's block
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
}  // namespace

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
}  // namespace ow

namespace ow {
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
ow_status velocity_refresh(ow_context *c, uint32_t mask);

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
// what every asynchronous form does between its argument checks and its first enqueue
ow_status begin_async(ow_context *c, int num_cascades) {
    if (ow_status st = refuse_faulted(c, layer_mask(num_cascades)); st != OW_OK) return st;
    OW_HIP(hipSetDevice(c->device));
    return OW_OK;
}
}  // namespace

extern "C" {

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

}  // extern "C"

namespace ow {
ow_status resolve_buoyancy_options(const ow_buoyancy_options *o, QueryParams *qp, BuoyancyParams *bp) {
    if (ow_status st = resolve_query_options(o ? &o->query : nullptr, qp); st != OW_OK) return st;
    bp->density = kDefaultDensity;
    bp->water_level = 0.0f;
    bp->warm_start = 0;
    bp->water_velocity = 0;
    float gravity = kDefaultGravity;
    if (o) {
        if (!std::isfinite(o->density) || !std::isfinite(o->gravity) || !std::isfinite(o->water_level))
            return fail(OW_ERR_INVALID, "density, gravity and water_level must be finite");
        if (o->flags & ~(OW_BUOYANCY_WARM_START | OW_BUOYANCY_WATER_VELOCITY)) return fail(OW_ERR_INVALID, "unknown buoyancy flags 0x%x", o->flags);
        if (o->density > 0.0f) bp->density = o->density;
        if (o->gravity > 0.0f) gravity = o->gravity;
        bp->water_level = o->water_level;
        bp->warm_start = (o->flags & OW_BUOYANCY_WARM_START) ? 1 : 0;
        bp->water_velocity = (o->flags & OW_BUOYANCY_WATER_VELOCITY) ? 1 : 0;
    }
    bp->gravity = gravity;
    bp->rho_g = bp->density * gravity;
    if (!std::isfinite(bp->rho_g)) return fail(OW_ERR_INVALID, "density * gravity overflows");
    return OW_OK;
}

ow_status check_buoyancy_arrays(const ow_buoyancy_body *bodies, int num_bodies, const ow_hull_point *hull, int num_points) {
    for (int b = 0; b < num_bodies; ++b) {
        const ow_buoyancy_body &B = bodies[b];
        if (B.point_offset < 0 || B.point_count < 0 || (int64_t)B.point_offset + B.point_count > num_points)
            return fail(OW_ERR_INVALID, "body %d: point range [%d, %d + %d) outside [0, %d)", b, B.point_offset, B.point_offset, B.point_count, num_points);
        for (int i = B.point_offset; i < B.point_offset + B.point_count; ++i)
            if (hull[i].body != b) return fail(OW_ERR_INVALID, "hull point %d lies in body %d's range but names body %d", i, b, hull[i].body);
    }
    for (int i = 0; i < num_points; ++i) {
        const ow_hull_point &h = hull[i];
        if (h.body < 0 || h.body >= num_bodies) return fail(OW_ERR_INVALID, "hull point %d: body %d outside [0, %d)", i, h.body, num_bodies);
        const ow_buoyancy_body &B = bodies[h.body];
        if (i < B.point_offset || i >= B.point_offset + B.point_count)
            return fail(OW_ERR_INVALID, "hull point %d names body %d, whose range does not hold it", i, h.body);
        if (!(h.volume >= 0.0f) || !(h.half_height >= 0.0f))
            return fail(OW_ERR_INVALID, "hull point %d: volume and half_height must be >= 0", i);
    }
    return OW_OK;
}

ow_status buoyancy_round_trip(const MapsView &v, DeviceScratch &scratch, const ow_buoyancy_body *bodies, int num_bodies, const ow_hull_point *hull,
                              int num_points, const float *map_scales, int num_cascades, const QueryParams &qp, const BuoyancyParams &bp,
                              ow_buoyancy_result *results, ow_buoyancy_point *points_inout, const u16x4 *vel) {
    Layout L;
    const size_t b_off = L.take((size_t)num_bodies * sizeof(BuoyancyBody)), h_off = L.take((size_t)num_points * sizeof(HullPoint));
    const size_t p_off = L.take((size_t)num_points * sizeof(BuoyancyPoint)), r_off = L.take((size_t)num_bodies * sizeof(BuoyancyResult));
    if (ow_status st = scratch.ensure(L.total, (size_t)1 << 20, 1, "bytes of buoyancy scratch"); st != OW_OK) return st;
    hipStream_t s = v.stream;
    char *base = (char *)scratch.ptr;
    BuoyancyBody *bd = (BuoyancyBody *)(base + b_off);
    HullPoint *hd = (HullPoint *)(base + h_off);
    BuoyancyPoint *pd = (BuoyancyPoint *)(base + p_off);
    BuoyancyResult *rd = (BuoyancyResult *)(base + r_off);
    if (num_bodies > 0) OW_HIP(hipMemcpyAsync(bd, bodies, (size_t)num_bodies * sizeof(BuoyancyBody), hipMemcpyHostToDevice, s));
    if (num_points > 0) OW_HIP(hipMemcpyAsync(hd, hull, (size_t)num_points * sizeof(HullPoint), hipMemcpyHostToDevice, s));
    if (bp.warm_start && num_points > 0) OW_HIP(hipMemcpyAsync(pd, points_inout, (size_t)num_points * sizeof(BuoyancyPoint), hipMemcpyHostToDevice, s));
    OW_HIP(launch_buoyancy(v.n, num_cascades, v.buf, bd, num_bodies, hd, num_points, surface_scales(map_scales, num_cascades), qp, bp, pd, rd, s, vel));
    if (num_bodies > 0) OW_HIP(hipMemcpyAsync(results, rd, (size_t)num_bodies * sizeof(BuoyancyResult), hipMemcpyDeviceToHost, s));
    if (points_inout && num_points > 0) OW_HIP(hipMemcpyAsync(points_inout, pd, (size_t)num_points * sizeof(BuoyancyPoint), hipMemcpyDeviceToHost, s));
    return OW_OK;
}
}  // namespace ow

namespace {
// ---- the velocity layers (ow_velocity_kernels.h) -------------------------------------------------------------------------------------
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

// what both context forms check before they touch the context's device: counts, options, pointers (host arrays: ranges and indices)
ow_status check_buoyancy_call(const ow_buoyancy_body *bodies, int32_t num_bodies, const ow_hull_point *hull, int32_t num_points,
                              const float *map_scales, const ow_buoyancy_options *opts, const void *results, const void *points, bool host,
                              ow::QueryParams *qp, ow::BuoyancyParams *bp) {
    if (num_bodies < 0 || num_points < 0) return fail(OW_ERR_INVALID, "num_bodies and num_points must be >= 0");
    if (ow_status st = ow::resolve_buoyancy_options(opts, qp, bp); st != OW_OK) return st;
    if (!map_scales || (num_bodies > 0 && (!bodies || !results)) || (num_points > 0 && !hull)) return fail(OW_ERR_INVALID, "null argument");
    if (num_points > 0 && !points && (bp->warm_start || !host))
        return fail(OW_ERR_INVALID, host ? "OW_BUOYANCY_WARM_START needs points_inout" : "points_dev is required");
    if (host) return ow::check_buoyancy_arrays(bodies, num_bodies, hull, num_points);
    return OW_OK;
}
}  // namespace

extern "C" {

ow_status ow_buoyancy(ow_context *c, const ow_buoyancy_body *bodies, int32_t num_bodies, const ow_hull_point *hull, int32_t num_points,
                      const float *map_scales, int32_t num_cascades, const ow_buoyancy_options *opts, ow_buoyancy_result *results,
                      ow_buoyancy_point *points_inout) {
    static_assert(sizeof(ow_buoyancy_body) == sizeof(ow::BuoyancyBody) && sizeof(ow_hull_point) == sizeof(ow::HullPoint) &&
                      sizeof(ow_buoyancy_point) == sizeof(ow::BuoyancyPoint) && sizeof(ow_buoyancy_result) == sizeof(ow::BuoyancyResult) &&
                      offsetof(ow_buoyancy_point, body) == offsetof(ow::BuoyancyPoint, body) &&
                      offsetof(ow_buoyancy_result, max_residual) == offsetof(ow::BuoyancyResult, max_residual) &&
                      offsetof(ow_buoyancy_body, point_offset) == offsetof(ow::BuoyancyBody, point_offset),
                  "record layout");
    ow::QueryParams qp;
    ow::BuoyancyParams bp;
    if (ow_status st = check_buoyancy_call(bodies, num_bodies, hull, num_points, map_scales, opts, results, points_inout, true, &qp, &bp); st != OW_OK)
        return st;
    if (ow_status st = check_point_query(c, 0, num_cascades); st != OW_OK) return st;
    if (num_bodies == 0 && num_points == 0) return OW_OK;
    OW_HIP(hipSetDevice(c->device));
    if (bp.water_velocity)  // the velocity layers the drag is taken against, refreshed in stream order first
        if (ow_status st = velocity_refresh(c, layer_mask(num_cascades)); st != OW_OK) return st;
    if (ow_status st = ow::buoyancy_round_trip(view_of(c), c->buoy_scratch, bodies, num_bodies, hull, num_points, map_scales, num_cascades, qp, bp, results,
                                               points_inout, bp.water_velocity ? c->vel : nullptr);
        st != OW_OK)
        return st;
    return sync_stream(c, layer_mask(num_cascades));
}

ow_status ow_buoyancy_async(ow_context *c, const ow_buoyancy_body *bodies_dev, int32_t num_bodies, const ow_hull_point *hull_dev,
                            int32_t num_points, const float *map_scales, int32_t num_cascades, const ow_buoyancy_options *opts,
                            ow_buoyancy_result *results_dev, ow_buoyancy_point *points_dev) {
    ow::QueryParams qp;
    ow::BuoyancyParams bp;
    if (ow_status st = check_buoyancy_call(bodies_dev, num_bodies, hull_dev, num_points, map_scales, opts, results_dev, points_dev, false, &qp, &bp);
        st != OW_OK)
        return st;
    if (ow_status st = check_point_query(c, 0, num_cascades); st != OW_OK) return st;
    if (num_bodies == 0 && num_points == 0) return OW_OK;
    if (ow_status st = begin_async(c, num_cascades); st != OW_OK) return st;
    if (bp.water_velocity)
        if (ow_status st = velocity_refresh(c, layer_mask(num_cascades)); st != OW_OK) return st;
    const ow::MapsView v = view_of(c);
    OW_HIP(ow::launch_buoyancy(v.n, num_cascades, v.buf, (const ow::BuoyancyBody *)bodies_dev, num_bodies, (const ow::HullPoint *)hull_dev, num_points,
                               surface_scales(map_scales, num_cascades), qp, bp, (ow::BuoyancyPoint *)points_dev, (ow::BuoyancyResult *)results_dev, v.stream,
                               bp.water_velocity ? c->vel : nullptr));
    return OW_OK;
}

}  // extern "C"

// ---- floating bodies (ow_rigid.h; kernels in ow_consumer.hip) ---------------------------------------------------------------------------

namespace {
// THE SELECTION RULE.  The fused kernel serialises ceil(point_count / 64) height solves per lane and substep and fills the chip with one wave
// per body; the split form runs one lane per hull point and pays two launches per substep.  Measured per frame of 4 substeps on 1024^2 x 4 maps
// (profiles/bodies_step.txt): with hulls of 16 points fused takes 0.72 - 0.80 of split's time for 1 .. 4096 bodies, with 64 points 0.84 - 0.96
// (inside the run-to-run spread for most counts); from 256 points on split takes 0.59 down to 0.05 of fused's time at every body count; at
// 16384 bodies split is ahead at 16 and 64 points too (0.86, 0.82).  The table has no rows between 64 and 256 points nor between 4096 and
// 16384 bodies: the thresholds are the last rows where fused was not behind.
constexpr int kBodiesFusedMaxPoints = 64;    // largest hull of the set, in points
constexpr int kBodiesFusedMaxBodies = 4096;  // body count
bool bodies_fused(const ow_context *c, const ow_bodies *set) {
    if (c->bodies_mode) return c->bodies_mode == 1;
    return set->max_points <= kBodiesFusedMaxPoints && set->A.num_bodies <= kBodiesFusedMaxBodies;
}

// the checks of ow_bodies_create / ow_bodies_set_state on the states themselves; range: per body offset, count to hold them to (or nullptr)
ow_status check_rigid_records(const ow_rigid_body *bodies, int first, int count, const int32_t *range) {
    for (int k = 0; k < count; ++k) {
        const ow_rigid_body &B = bodies[k];
        const int b = first + k;
        const double *groups[] = {B.position, B.linear_velocity, B.angular_velocity, B.inverse_inertia, B.applied_force, B.applied_torque};
        for (const double *g : groups)
            for (int i = 0; i < 3; ++i)
                if (!std::isfinite(g[i])) return fail(OW_ERR_INVALID, "body %d: state, mass properties and applied loads must be finite", b);
        if (!std::isfinite(B.mass) || !std::isfinite(B.linear_drag) || !std::isfinite(B.quadratic_drag))
            return fail(OW_ERR_INVALID, "body %d: mass and drag must be finite", b);
        for (int i = 0; i < 3; ++i)
            if (B.inverse_inertia[i] < 0.0) return fail(OW_ERR_INVALID, "body %d: inverse_inertia must be >= 0", b);
        double n2 = 0.0;
        for (int i = 0; i < 4; ++i) {
            if (!std::isfinite(B.orientation[i])) return fail(OW_ERR_INVALID, "body %d: orientation must be a finite unit quaternion", b);
            n2 += B.orientation[i] * B.orientation[i];
        }
        if (!(std::fabs(std::sqrt(n2) - 1.0) <= 1e-6)) return fail(OW_ERR_INVALID, "body %d: orientation must be a unit quaternion (|q| = %.9g)", b, std::sqrt(n2));
        if (B.reserved[0] != 0u || B.reserved[1] != 0u) return fail(OW_ERR_INVALID, "body %d: ow_rigid_body.reserved must be 0", b);
        if (range && (B.point_offset != range[2 * b] || B.point_count != range[2 * b + 1]))
            return fail(OW_ERR_INVALID, "body %d: the hull range [%d, %d + %d) is fixed at ow_bodies_create", b, range[2 * b], range[2 * b], range[2 * b + 1]);
    }
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
ow_status check_bodies_handle(const ow_context *c, const ow_bodies *set) { return check_handle(c, set, "body set"); }
ow_status check_bodies_span(const ow_context *c, const ow_bodies *set, int32_t first, int32_t count, const void *records) {
    if (ow_status st = check_bodies_handle(c, set); st != OW_OK) return st;
    if (first < 0 || count < 0 || (int64_t)first + count > set->A.num_bodies)
        return fail(OW_ERR_INVALID, "bodies [%d, %d + %d) outside [0, %d)", first, first, count, set->A.num_bodies);
    if (count > 0 && !records) return fail(OW_ERR_INVALID, "null argument");
    return OW_OK;
}
}  // namespace

extern "C" {

ow_status ow_bodies_create(ow_context *c, const ow_rigid_body *bodies, int32_t num_bodies, const ow_hull_point *hull, int32_t num_points, ow_bodies **out) {
    static_assert(sizeof(ow_rigid_body) == sizeof(ow::RigidBody) && offsetof(ow_rigid_body, orientation) == offsetof(ow::RigidBody, orientation) &&
                      offsetof(ow_rigid_body, mass) == offsetof(ow::RigidBody, mass) &&
                      offsetof(ow_rigid_body, inverse_inertia) == offsetof(ow::RigidBody, inverse_inertia) &&
                      offsetof(ow_rigid_body, applied_torque) == offsetof(ow::RigidBody, applied_torque) &&
                      offsetof(ow_rigid_body, linear_drag) == offsetof(ow::RigidBody, linear_drag) &&
                      offsetof(ow_rigid_body, point_offset) == offsetof(ow::RigidBody, point_offset),
                  "record layout");
    if (!out) return fail(OW_ERR_INVALID, "null argument");
    *out = nullptr;
    if (num_bodies < 1 || num_points < 0) return fail(OW_ERR_INVALID, "num_bodies must be >= 1 and num_points >= 0");
    if (!bodies || (num_points > 0 && !hull)) return fail(OW_ERR_INVALID, "null argument");
    std::vector<ow_buoyancy_body> ranges((size_t)num_bodies);
    std::vector<int32_t> range((size_t)num_bodies * 2);
    int max_points = 0;
    for (int b = 0; b < num_bodies; ++b) {
        std::memset(&ranges[b], 0, sizeof(ow_buoyancy_body));
        ranges[b].point_offset = range[2 * b] = bodies[b].point_offset;
        ranges[b].point_count = range[2 * b + 1] = bodies[b].point_count;
        max_points = std::max(max_points, bodies[b].point_count);
    }
    if (ow_status st = ow::check_buoyancy_arrays(ranges.data(), num_bodies, hull, num_points); st != OW_OK) return st;
    for (int i = 0; i < num_points; ++i)
        if (!std::isfinite(hull[i].volume) || !std::isfinite(hull[i].half_height) || !std::isfinite(hull[i].local[0]) || !std::isfinite(hull[i].local[1]) ||
            !std::isfinite(hull[i].local[2]))
            return fail(OW_ERR_INVALID, "hull point %d: local, volume and half_height must be finite", i);
    if (ow_status st = check_rigid_records(bodies, 0, num_bodies, nullptr); st != OW_OK) return st;
    if (!c) return fail(OW_ERR_INVALID, "null context");
    const size_t nb = (size_t)num_bodies, np = (size_t)num_points;
    Layout L;
    const size_t s_off = L.take(nb * sizeof(ow::RigidBody)), b_off = L.take(nb * sizeof(ow::BuoyancyBody)), h_off = L.take(np * sizeof(ow::HullPoint));
    const size_t p_off = L.take(np * sizeof(ow::BuoyancyPoint)), r_off = L.take(nb * sizeof(ow::BuoyancyResult)), f_off = L.take(nb * sizeof(int32_t));
    ow_bodies *set;
    if (ow_status st = new_handle(c, L.total, "body set", &set); st != OW_OK) return st;
    char *base = (char *)set->block;
    set->A.state = (ow::RigidBody *)(base + s_off);
    set->A.records = (ow::BuoyancyBody *)(base + b_off);
    set->A.hull = (const ow::HullPoint *)(base + h_off);
    set->A.pts = (ow::BuoyancyPoint *)(base + p_off);
    set->A.results = (ow::BuoyancyResult *)(base + r_off);
    set->A.flags = (int32_t *)(base + f_off);
    set->A.num_bodies = num_bodies;
    set->A.num_points = num_points;
    set->max_points = max_points;
    set->range = std::move(range);
    hipStream_t s = main_stream(c);
    const bool enqueued = hipMemsetAsync(set->block, 0, L.total, s) == hipSuccess &&
                          hipMemcpyAsync(set->A.state, bodies, nb * sizeof(ow::RigidBody), hipMemcpyHostToDevice, s) == hipSuccess &&
                          (np == 0 || hipMemcpyAsync((void *)set->A.hull, hull, np * sizeof(ow::HullPoint), hipMemcpyHostToDevice, s) == hipSuccess) &&
                          ow::launch_bodies_pose(set->A, 0, num_bodies, s) == hipSuccess;
    return finish_create(c, set, s, enqueued, "body set upload", out);
}

void ow_bodies_destroy(ow_context *, ow_bodies *set) {
    if (set) release_handle(set);
    delete set;
}

ow_status ow_bodies_step(ow_context *c, ow_bodies *set, const float *map_scales, int32_t num_cascades, const ow_bodies_options *opts, int32_t substeps,
                         double dt) {
    if (substeps < 1 || substeps > OW_BODIES_MAX_SUBSTEPS) return fail(OW_ERR_INVALID, "substeps %d outside [1,%d]", substeps, OW_BODIES_MAX_SUBSTEPS);
    if (!std::isfinite(dt) || !(dt > 0.0)) return fail(OW_ERR_INVALID, "dt must be finite and > 0");
    ow::QueryParams qp;
    ow::BuoyancyParams bp;
    if (ow_status st = ow::resolve_buoyancy_options(opts ? &opts->buoyancy : nullptr, &qp, &bp); st != OW_OK) return st;
    if (opts)
        if (ow_status st = check_reserved(opts->reserved, "ow_bodies_options"); st != OW_OK) return st;
    if (!map_scales) return fail(OW_ERR_INVALID, "null argument");
    if (ow_status st = check_bodies_handle(c, set); st != OW_OK) return st;
    if (ow_status st = check_point_query(c, 0, num_cascades); st != OW_OK) return st;
    if (ow_status st = begin_async(c, num_cascades); st != OW_OK) return st;
    if (bp.water_velocity)  // once per call: the maps do not move between the substeps of a call
        if (ow_status st = velocity_refresh(c, layer_mask(num_cascades)); st != OW_OK) return st;
    ow::RigidParams rp;
    rp.dt = dt;
    rp.gravity = (double)bp.gravity;  // the g of rho_g: weight and buoyancy use the same one
    const bool fused = bodies_fused(c, set);
    const ow::MapsView v = view_of(c);
    OW_HIP(ow::launch_bodies_step(v.n, num_cascades, v.buf, set->A, surface_scales(map_scales, num_cascades), qp, bp, rp, substeps, fused, v.stream,
                                  bp.water_velocity ? c->vel : nullptr));
    set->substeps += (uint64_t)substeps;
    (fused ? set->fused_launches : set->split_calls) += 1;
    return OW_OK;
}

ow_status ow_bodies_get_state(ow_context *c, ow_bodies *set, int32_t first, int32_t count, ow_rigid_body *records) {
    if (ow_status st = check_bodies_span(c, set, first, count, records); st != OW_OK) return st;
    return read_back(c, records, set->A.state + first, (size_t)count * sizeof(ow::RigidBody));
}

ow_status ow_bodies_set_state(ow_context *c, ow_bodies *set, int32_t first, int32_t count, const ow_rigid_body *records) {
    if (ow_status st = check_bodies_span(c, set, first, count, records); st != OW_OK) return st;
    if (ow_status st = check_rigid_records(records, first, count, set->range.data()); st != OW_OK) return st;
    OW_HIP(hipSetDevice(c->device));
    if (ow_status st = sync_stream(c, 0); st != OW_OK) return st;
    if (count == 0) return OW_OK;
    OW_HIP(hipMemcpy(set->A.state + first, records, (size_t)count * sizeof(ow::RigidBody), hipMemcpyHostToDevice));
    OW_HIP(ow::launch_bodies_pose(set->A, first, count, main_stream(c)));
    ++c->host_syncs;
    OW_HIP(hipStreamSynchronize(main_stream(c)));
    return OW_OK;
}

ow_status ow_bodies_get_results(ow_context *c, ow_bodies *set, int32_t first, int32_t count, ow_buoyancy_result *results) {
    if (ow_status st = check_bodies_span(c, set, first, count, results); st != OW_OK) return st;
    return read_back(c, results, set->A.results + first, (size_t)count * sizeof(ow::BuoyancyResult));
}

ow_status ow_bodies_get_device_ptrs(ow_context *c, ow_bodies *set, void **bodies_dev, void **results_dev, void **points_dev) {
    if (ow_status st = check_bodies_handle(c, set); st != OW_OK) return st;
    if (bodies_dev) *bodies_dev = set->A.records;
    if (results_dev) *results_dev = set->A.results;
    if (points_dev) *points_dev = set->A.pts;
    return OW_OK;
}

ow_status ow_sync_stats(const ow_context *c, uint64_t *host_syncs) {
    if (!c || !host_syncs) return fail(OW_ERR_INVALID, "null argument");
    *host_syncs = c->host_syncs;
    return OW_OK;
}

ow_status ow_bodies_stats(ow_context *c, ow_bodies *set, uint64_t *substeps, uint64_t *fused_launches, uint64_t *split_calls, uint64_t *faulted_bodies) {
    if (ow_status st = check_bodies_handle(c, set); st != OW_OK) return st;
    if (faulted_bodies) {
        std::vector<int32_t> flags((size_t)set->A.num_bodies);
        if (ow_status st = read_back(c, flags.data(), set->A.flags, flags.size() * sizeof(int32_t)); st != OW_OK) return st;
        uint64_t n = 0;
        for (int32_t f : flags) n += f != 0;
        *faulted_bodies = n;
    }
    if (substeps) *substeps = set->substeps;
    if (fused_launches) *fused_launches = set->fused_launches;
    if (split_calls) *split_calls = set->split_calls;
    return OW_OK;
}

}  // extern "C"

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

// the per-cascade bound words of the slab on the current device, allocated by the first call that needs them
ow_status ray_bound_words(uint32_t **bound) {
    if (!*bound && hipMalloc((void **)bound, OW_MAX_CASCADES * sizeof(uint32_t)) != hipSuccess) {
        *bound = nullptr;
        return fail(OW_ERR_NOMEM, "hipMalloc failed for the ray-cast bound words");
    }
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
    if (ow_status st = ow::ray_bound_words(&c->ray_bound); st != OW_OK) return st;
    const ow::MapsView v = view_of(c);
    OW_HIP(ow::launch_raycast(v.n, num_cascades, v.buf, (const ow::Ray *)rays_dev, count, surface_scales(map_scales, num_cascades), rp, c->ray_bound,
                              (ow::RaycastHit *)out_dev, v.stream));
    return OW_OK;
}

}  // extern "C"

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

// ow_render_options (NULL = the defaults) -> the hit's settings and the shading's; the uniform-only constants in FP64, narrowed once
ow_status resolve_render_options(const ow_render_options *opts, ow::RaycastParams *rp, ow::ShadeParams *sp) {
    ow_render_options def;
    if (!opts) {
        render_defaults(&def);
        opts = &def;
    }
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
ow_status check_pixel_alignment(const void *rgba8_dev, const void *pixels_dev) {
    if (((uintptr_t)rgba8_dev & 3u) || ((uintptr_t)pixels_dev & 15u)) return fail(OW_ERR_INVALID, "rgba8_dev must be 4-byte and pixels_dev 16-byte aligned");
    return OW_OK;
}

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
// Launches already enqueued (the asynchronous forms) may still read a scratch block that exists and has to grow to `need` bytes: one counted
// synchronisation through main_stream before DeviceScratch::ensure replaces it.
ow_status sync_before_growth(ow_context *c, const ow::DeviceScratch &scratch, size_t need) {
    if (scratch.ptr && need > scratch.bytes) {
        ++c->host_syncs;
        OW_HIP(hipStreamSynchronize(main_stream(c)));
    }
    return OW_OK;
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
    if (ow_status st = ow::ray_bound_words(&c->ray_bound); st != OW_OK) return st;
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
    if (ow_status st = ow::ray_bound_words(&c->ray_bound); st != OW_OK) return st;
    return view_enqueue(c, cp, map_scales, num_cascades, rp, sp, (uint32_t *)rgba8_dev, (ow::RenderPixel *)pixels_dev);
}

}  // extern "C"

namespace {
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

// the synchronous forms: picture_round_trip with the records uploaded first and no layer to refuse (the draw reads no map)
ow_status billboard_round_trip(ow_context *c, const ow::CameraParams &cp, const ow::SprayDrawParams &dp, int bin_side, const ow_spray *e,
                               const ow_spray_instance *upload, uint32_t slots, ow_render_pixel *pixels_inout, void *rgba8_out) {
    OW_HIP(hipSetDevice(c->device));
    return picture_round_trip(c, (size_t)cp.width * cp.height, rgba8_out, pixels_inout, true, 0, [&](uint32_t *rgba_dev, ow::RenderPixel *pixels_dev) {
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
    return billboard_round_trip(c, cp, dp, bin_side, e, nullptr, e->P.amount, pixels_inout, rgba8_out);
}

ow_status ow_billboard_draw_async(ow_context *c, ow_spray *e, ow_billboard_material *m, const ow_camera *camera, const ow_billboard_draw_options *opts,
                                  ow_render_pixel *pixels_dev, void *rgba8_dev) {
    ow::CameraParams cp;
    ow::SprayDrawParams dp;
    int bin_side;
    if (ow_status st = check_billboard_draw(c, m, camera, opts, pixels_dev, rgba8_dev, &cp, &dp, &bin_side); st != OW_OK) return st;
    if (ow_status st = check_handle(c, e, "spray emitter"); st != OW_OK) return st;
    if (ow_status st = check_pixel_alignment(rgba8_dev, pixels_dev); st != OW_OK) return st;
    OW_HIP(hipSetDevice(c->device));
    dp.time = (float)e->H.time;
    return billboard_enqueue(c, cp, dp, bin_side, e, nullptr, e->P.amount, (ow::RenderPixel *)pixels_dev, (uint32_t *)rgba8_dev);
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
    return billboard_round_trip(c, cp, dp, bin_side, nullptr, instances, (uint32_t)count, pixels_inout, rgba8_out);
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
    if (!opts) {
        solid_defaults(&def);
        opts = &def;
    }
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
// the number of instances of one draw against the shape
ow_status check_solid_count(const ow_solid *solid, int64_t count) {
    if (count < 0 || count > OW_SOLID_MAX_INSTANCES) return fail(OW_ERR_INVALID, "%lld instances outside [0,%d]", (long long)count, OW_SOLID_MAX_INSTANCES);
    if (count * solid->shape.num_triangles > ow::kSolidMaxProduct || count * solid->shape.num_vertices > ow::kSolidMaxProduct)
        return fail(OW_ERR_INVALID, "%lld instances of %d triangles and %d vertices: more than 2^24 per draw", (long long)count, solid->shape.num_triangles,
                    solid->shape.num_vertices);
    return OW_OK;
}
ow_status check_solid_bodies(const ow_context *c, const ow_solid *solid, const ow_bodies *set, int32_t first, int32_t count) {
    if (ow_status st = check_bodies_handle(c, set); st != OW_OK) return st;
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

// the synchronous forms: picture_round_trip with the records uploaded first and no layer to refuse (the draw reads no map)
ow_status solid_round_trip(ow_context *c, const ow_solid *solid, const ow::CameraParams &cp, const ow::SolidParams &sp, const ow_bodies *set, int first,
                           const float *upload, int count, ow_render_pixel *pixels_inout, void *rgba8_out) {
    OW_HIP(hipSetDevice(c->device));
    return picture_round_trip(c, (size_t)cp.width * cp.height, rgba8_out, pixels_inout, true, 0, [&](uint32_t *rgba_dev, ow::RenderPixel *pixels_dev) {
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
    const size_t l_off = L.take(nv * 3 * sizeof(float)), i_off = L.take(nt * 3 * sizeof(int32_t));
    ow_solid *m;
    if (ow_status st = new_handle(c, L.total, "solid", &m); st != OW_OK) return st;
    char *base = (char *)m->block;
    m->shape = ow::SolidShape{(const float *)(base + l_off), (const int32_t *)(base + i_off), num_vertices, num_triangles};
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
    return solid_round_trip(c, solid, cp, sp, bodies, first_body, nullptr, body_count, pixels_inout, rgba8_out);
}

ow_status ow_solid_draw_async(ow_context *c, ow_solid *solid, ow_bodies *bodies, int32_t first_body, int32_t body_count, const ow_camera *camera,
                              const ow_solid_options *opts, ow_render_pixel *pixels_dev, void *rgba8_dev) {
    ow::CameraParams cp;
    ow::SolidParams sp;
    if (ow_status st = check_solid_draw(c, solid, camera, opts, pixels_dev, rgba8_dev, &cp, &sp); st != OW_OK) return st;
    if (ow_status st = check_solid_bodies(c, solid, bodies, first_body, body_count); st != OW_OK) return st;
    if (ow_status st = check_pixel_alignment(rgba8_dev, pixels_dev); st != OW_OK) return st;
    OW_HIP(hipSetDevice(c->device));
    return solid_enqueue(c, solid, cp, sp, bodies, first_body, nullptr, body_count, (ow::RenderPixel *)pixels_dev, (uint32_t *)rgba8_dev);
}

ow_status ow_solid_draw_instances(ow_context *c, ow_solid *solid, const float *transforms, int32_t count, const ow_camera *camera,
                                  const ow_solid_options *opts, ow_render_pixel *pixels_inout, void *rgba8_out) {
    if (count < 0 || count > OW_SOLID_MAX_INSTANCES) return fail(OW_ERR_INVALID, "count %d outside [0,%d]", count, OW_SOLID_MAX_INSTANCES);
    if (count > 0 && !transforms) return fail(OW_ERR_INVALID, "null argument");
    ow::CameraParams cp;
    ow::SolidParams sp;
    if (ow_status st = check_solid_draw(c, solid, camera, opts, pixels_inout, rgba8_out, &cp, &sp); st != OW_OK) return st;
    if (ow_status st = check_solid_count(solid, count); st != OW_OK) return st;
    return solid_round_trip(c, solid, cp, sp, nullptr, 0, transforms, count, pixels_inout, rgba8_out);
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
bool in_range(float v, float lo, float hi) { return v >= lo && v <= hi; }  // false for a NaN

ow_status check_sky_options(const ow_sky_options *o) {
    static_assert(sizeof(ow_sky_options) == sizeof(ow::SkyOptions) && offsetof(ow_sky_options, energy) == offsetof(ow::SkyOptions, energy) &&
                      OW_SKY_MAX_SIDE == ow::kSkyMaxSide,
                  "record layout");
    if (o->srgb > 1u) return fail(OW_ERR_INVALID, "ow_sky_options: srgb is not 0 or 1");
    if (!in_range(o->energy, 0.0f, ow::kEnvColorMax)) return fail(OW_ERR_INVALID, "ow_sky_options: energy outside [0,1e12]");
    return check_reserved(o->reserved, "ow_sky_options");
}

// ow_environment_options (NULL = the defaults) -> the pass's constants; the sky's are filled in by check_environment
ow_status resolve_environment_options(const ow_environment_options *opts, ow::EnvParams *ep) {
    static_assert(sizeof(ow_environment_options) == sizeof(ow::EnvironmentOptions) &&
                      offsetof(ow_environment_options, flags) == offsetof(ow::EnvironmentOptions, flags) &&
                      offsetof(ow_environment_options, sun_direction) == offsetof(ow::EnvironmentOptions, sun_direction) &&
                      offsetof(ow_environment_options, reserved) == offsetof(ow::EnvironmentOptions, reserved) && OW_RAY_ENVIRONMENT == ow::kRayEnvironment &&
                      OW_FOG_EXPONENTIAL == ow::kFogExponential && OW_FOG_DEPTH == ow::kFogDepth,
                  "record layout");
    ow_environment_options def;
    if (!opts) {
        environment_defaults(&def);
        opts = &def;
    }
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

// the argument checks both forms of the pass share: ow_solid_draw's, in its order, then the context and the sky
ow_status check_environment(const ow_context *c, const ow_sky *sky, const ow_camera *camera, const ow_environment_options *opts, const void *pixels,
                            ow::CameraParams *cp, ow::EnvParams *ep) {
    if (!pixels) return fail(OW_ERR_INVALID, "null argument: the records");
    if (ow_status st = resolve_camera(camera, cp); st != OW_OK) return st;
    if (ow_status st = resolve_environment_options(opts, ep); st != OW_OK) return st;
    if (!c) return fail(OW_ERR_INVALID, "null context");
    if (sky) {
        if (ow_status st = check_handle(c, sky, "sky"); st != OW_OK) return st;
        ep->has_sky = 1;
        ep->sky = sky->tex;
        ep->srgb = sky->srgb;
        ep->energy = sky->energy;
    }
    ep->camera_ok = ow::mesh_camera_ok(*cp) ? 1 : 0;
    return OW_OK;
}

// ow_present_options (NULL = the defaults) -> the present's constants and the output's size
ow_status resolve_present_options(const ow_present_options *opts, const ow::CameraParams &cp, ow::PresentParams *pp, int *out_width, int *out_height) {
    static_assert(sizeof(ow_present_options) == sizeof(ow::PresentOptions) && offsetof(ow_present_options, srgb) == offsetof(ow::PresentOptions, srgb) &&
                      offsetof(ow_present_options, reserved) == offsetof(ow::PresentOptions, reserved) &&
                      OW_PRESENT_MAX_DOWNSAMPLE == ow::kPresentMaxDownsample && OW_TONEMAP_LINEAR == ow::kTonemapLinear &&
                      OW_TONEMAP_REINHARD == ow::kTonemapReinhard && OW_TONEMAP_FILMIC == ow::kTonemapFilmic,
                  "record layout");
    ow_present_options def;
    if (!opts) {
        present_defaults(&def);
        opts = &def;
    }
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
    if (!opts) {
        sky_defaults(&def);
        opts = &def;
    }
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
    ow::CameraParams cp;
    ow::EnvParams ep;
    if (ow_status st = check_environment(c, sky, camera, opts, pixels_inout, &cp, &ep); st != OW_OK) return st;
    OW_HIP(hipSetDevice(c->device));
    return picture_round_trip(c, (size_t)cp.width * cp.height, nullptr, pixels_inout, true, 0, [&](uint32_t *, ow::RenderPixel *pixels_dev) {
        OW_HIP(ow::launch_environment_apply(cp, ep, pixels_dev, main_stream(c)));
        return OW_OK;
    });
}

ow_status ow_environment_apply_async(ow_context *c, ow_sky *sky, const ow_camera *camera, const ow_environment_options *opts, ow_render_pixel *pixels_dev) {
    ow::CameraParams cp;
    ow::EnvParams ep;
    if (ow_status st = check_environment(c, sky, camera, opts, pixels_dev, &cp, &ep); st != OW_OK) return st;
    if (ow_status st = check_pixel_alignment(nullptr, pixels_dev); st != OW_OK) return st;
    OW_HIP(hipSetDevice(c->device));
    OW_HIP(ow::launch_environment_apply(cp, ep, (ow::RenderPixel *)pixels_dev, main_stream(c)));
    return OW_OK;
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
    if (!opts) {
        radiance_defaults(&def);
        opts = &def;
    }
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

// ow_radiance_light_options (NULL = the defaults) -> the pass's constants; the pyramid's are filled in by check_radiance_light
ow_status resolve_radiance_light_options(const ow_radiance_light_options *opts, ow::SkyLightParams *lp) {
    static_assert(sizeof(ow_radiance_light_options) == sizeof(ow::SkyLightOptions) &&
                      offsetof(ow_radiance_light_options, flags) == offsetof(ow::SkyLightOptions, flags) &&
                      offsetof(ow_radiance_light_options, reserved) == offsetof(ow::SkyLightOptions, reserved) && OW_RAY_SKY_LIT == ow::kRaySkyLit,
                  "record layout");
    ow_radiance_light_options def;
    if (!opts) {
        radiance_light_defaults(&def);
        opts = &def;
    }
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

// the argument checks both forms of the pass share: ow_environment_apply's, in its order, then the context and the pyramid
ow_status check_radiance_light(const ow_context *c, const ow_radiance *radiance, const ow_camera *camera, const ow_radiance_light_options *opts,
                               const void *pixels, ow::CameraParams *cp, ow::SkyLightParams *lp) {
    if (!pixels) return fail(OW_ERR_INVALID, "null argument: the records");
    if (ow_status st = resolve_camera(camera, cp); st != OW_OK) return st;
    if (ow_status st = resolve_radiance_light_options(opts, lp); st != OW_OK) return st;
    if (ow_status st = check_handle(c, radiance, "radiance pyramid"); st != OW_OK) return st;
    lp->levels = radiance->plan.levels;
    for (int k = 0; k < radiance->plan.levels; ++k) lp->R[k] = radiance->R[k];
    lp->E = radiance->E;
    lp->camera_ok = ow::mesh_camera_ok(*cp) ? 1 : 0;
    return OW_OK;
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
    ow::CameraParams cp;
    ow::SkyLightParams lp;
    if (ow_status st = check_radiance_light(c, radiance, camera, opts, pixels_inout, &cp, &lp); st != OW_OK) return st;
    OW_HIP(hipSetDevice(c->device));
    return picture_round_trip(c, (size_t)cp.width * cp.height, nullptr, pixels_inout, true, 0, [&](uint32_t *, ow::RenderPixel *pixels_dev) {
        OW_HIP(ow::launch_sky_light_apply(cp, lp, pixels_dev, main_stream(c)));
        return OW_OK;
    });
}

ow_status ow_radiance_light_apply_async(ow_context *c, ow_radiance *radiance, const ow_camera *camera, const ow_radiance_light_options *opts,
                                        ow_render_pixel *pixels_dev) {
    ow::CameraParams cp;
    ow::SkyLightParams lp;
    if (ow_status st = check_radiance_light(c, radiance, camera, opts, pixels_dev, &cp, &lp); st != OW_OK) return st;
    if (ow_status st = check_pixel_alignment(nullptr, pixels_dev); st != OW_OK) return st;
    OW_HIP(hipSetDevice(c->device));
    OW_HIP(ow::launch_sky_light_apply(cp, lp, (ow::RenderPixel *)pixels_dev, main_stream(c)));
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
    if (!opts) {
        shadow_defaults(&def);
        opts = &def;
    }
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

// the argument checks both forms of the pass share: ow_solid_draw's, in its order, then the context and the map
ow_status check_shadow_apply(const ow_context *c, const ow_shadow_map *map, const ow_camera *camera, const ow_shadow_options *opts, const void *pixels,
                             ow::CameraParams *cp, ow::ShadowApply *ap) {
    if (!pixels) return fail(OW_ERR_INVALID, "null argument: the records");
    if (ow_status st = resolve_camera(camera, cp); st != OW_OK) return st;
    if (ow_status st = resolve_shadow_options(opts, ap); st != OW_OK) return st;
    if (ow_status st = check_shadow_map(c, map); st != OW_OK) return st;
    ap->camera_ok = ow::mesh_camera_ok(*cp) ? 1 : 0;
    return OW_OK;
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
    ow::CameraParams cp;
    ow::ShadowApply ap;
    if (ow_status st = check_shadow_apply(c, map, camera, opts, pixels_inout, &cp, &ap); st != OW_OK) return st;
    OW_HIP(hipSetDevice(c->device));
    return picture_round_trip(c, (size_t)cp.width * cp.height, rgba8_out, pixels_inout, true, 0, [&](uint32_t *rgba_dev, ow::RenderPixel *pixels_dev) {
        OW_HIP(ow::launch_shadow_apply(map->map, cp, map->P, ap, pixels_dev, rgba_dev, main_stream(c)));
        return OW_OK;
    });
}

ow_status ow_shadow_apply_async(ow_context *c, ow_shadow_map *map, const ow_camera *camera, const ow_shadow_options *opts, ow_render_pixel *pixels_dev,
                                void *rgba8_dev) {
    ow::CameraParams cp;
    ow::ShadowApply ap;
    if (ow_status st = check_shadow_apply(c, map, camera, opts, pixels_dev, &cp, &ap); st != OW_OK) return st;
    if (ow_status st = check_pixel_alignment(rgba8_dev, pixels_dev); st != OW_OK) return st;
    OW_HIP(hipSetDevice(c->device));
    OW_HIP(ow::launch_shadow_apply(map->map, cp, map->P, ap, (ow::RenderPixel *)pixels_dev, (uint32_t *)rgba8_dev, main_stream(c)));
    return OW_OK;
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

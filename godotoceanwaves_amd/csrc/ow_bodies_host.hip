// ow_bodies_host.hip -- buoyancy and the floating bodies: ow_buoyancy (for a context and, through its round trip, a group: ow_internal.h),
// the ow_bodies_* body sets and their fused / split selection rule, and ow_sync_stats, over the kernels of ow_consumer.hip
// (ow_buoyancy.h, ow_rigid.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ow_consumer_host.h"

using namespace ow::readside;
using ow::fail, ow::layer_mask, ow::main_stream, ow::sync_stream;

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

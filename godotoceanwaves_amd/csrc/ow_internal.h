// ow_internal.h -- what the translation units of libocean_waves.so share besides the public header: error reporting, and the read side's
// host code that serves a context and a group alike (ow_points_host.hip, ow_bodies_host.hip; the scratch: ow_consumer_host.hip).
#pragma once
#include <hip/hip_runtime.h>

// The library is built with -fvisibility=hidden: only what include/ocean_waves.h declares is exported.
#pragma GCC visibility push(default)
#include "../../include/ocean_waves.h"
#pragma GCC visibility pop

#include "ow_kernels.h"

namespace ow {

// sets the calling thread's ow_last_error() text (printf-style) and returns `st` (ow_runtime.hip)
ow_status fail(ow_status st, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
// replaces the calling thread's ow_last_error() text (a group hands a worker thread's message to its caller; ow_runtime.hip)
void set_last_error(const char *message);
// every record finite, tile_length positive, time + delta finite (ow_schedule.hip; sets the error text)
ow_status validate_records(const ow_cascade_params *params, int count, double delta);
// the context's device status word without synchronising (ow_runtime.hip)
ow_status poll_status(ow_context *c);

// ---- the read side (points and rays: ow_points_host.hip; buoyancy: ow_bodies_host.hip) ----
// ow_query_options (NULL = defaults) -> the solver's settings, OW_ERR_INVALID for a value out of range
ow_status resolve_query_options(const ow_query_options *opts, QueryParams *qp);
// ow_buoyancy_options (NULL = defaults) -> the solver's settings and the model's constants
ow_status resolve_buoyancy_options(const ow_buoyancy_options *opts, QueryParams *qp, BuoyancyParams *bp);
// ow_raycast_options (NULL = defaults) -> the ray cast's settings, OW_ERR_INVALID for a value out of range
ow_status resolve_raycast_options(const ow_raycast_options *opts, RaycastParams *rp);
// the host-side checks of ow_buoyancy / ow_group_buoyancy on host arrays: ranges, body indices, volumes, half heights
ow_status check_buoyancy_arrays(const ow_buoyancy_body *bodies, int num_bodies, const ow_hull_point *hull, int num_points);

// A grow-only device allocation on the current device.  Nothing that reads the old block may be in flight when it grows: every user but three
// synchronises before it returns (the exceptions, the mesh draw's visibility words and the billboard and solid draws' blocks, synchronise before
// they grow: ow_consumer_host.h sync_before_growth).  Defined in ow_consumer_host.hip.
struct DeviceScratch {
    void *ptr = nullptr;
    size_t bytes = 0;  // capacity
    // at least `need` bytes; a block that has to grow is replaced by one of max(need, floor).  OW_ERR_NOMEM: "hipMalloc failed for <capacity / unit> <what>"
    ow_status ensure(size_t need, size_t floor, size_t unit, const char *what);
    void release();
};

// What a consumer launch needs from its owner: a context's own maps on its stream, or a group's gathered arrays on its root device.
struct MapsView {
    int n;
    DeviceBuffers buf;
    hipStream_t stream;
    int device;
};
// The synchronous calls' device halves on v.stream, with v.device current: grow-only scratch, the arrays in, the launches, the records out.
// The caller synchronises.  Points: the sampling kernel without qp, the velocity records with vel (the velocity layers), the query otherwise.
ow_status points_round_trip(const MapsView &v, DeviceScratch &scratch, const float *xz, int count, const float *map_scales, int num_cascades,
                            const QueryParams *qp, const u16x4 *vel, void *out);
// bound: the per-cascade bound words of the slab, allocated once (ow_consumer_host.h ray_bound_words)
ow_status rays_round_trip(const MapsView &v, DeviceScratch &scratch, uint32_t **bound, const ow_ray *rays, int count, const float *map_scales,
                          int num_cascades, const RaycastParams &rp, ow_raycast_hit *out);
// results and, with points_inout, the per-point records come back; vel: the velocity layers (OW_BUOYANCY_WATER_VELOCITY)
ow_status buoyancy_round_trip(const MapsView &v, DeviceScratch &scratch, const ow_buoyancy_body *bodies, int num_bodies, const ow_hull_point *hull,
                              int num_points, const float *map_scales, int num_cascades, const QueryParams &qp, const BuoyancyParams &bp,
                              ow_buoyancy_result *results, ow_buoyancy_point *points_inout, const u16x4 *vel = nullptr);

}  // namespace ow

#define OW_HIP(call)                                                                                       \
    do {                                                                                                   \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess) return ow::fail(OW_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

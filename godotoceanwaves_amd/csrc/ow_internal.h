// ow_internal.h -- what the translation units of libocean_waves.so share besides the public header: error reporting.
#pragma once
#include <hip/hip_runtime.h>

// The library is built with -fvisibility=hidden: only what include/ocean_waves.h declares is exported.
#pragma GCC visibility push(default)
#include "../../include/ocean_waves.h"
#pragma GCC visibility pop

namespace ow {

// sets the calling thread's ow_last_error() text (printf-style) and returns `st`
ow_status fail(ow_status st, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
// replaces the calling thread's ow_last_error() text (a group hands a worker thread's message to its caller)
void set_last_error(const char *message);
// every record finite, tile_length positive, time + delta finite (ow_runtime.hip; sets the error text)
ow_status validate_records(const ow_cascade_params *params, int count, double delta);
// the context's device status word without synchronising (ow_runtime.hip)
ow_status poll_status(ow_context *c);
// ow_query_options (NULL = defaults) -> the solver's settings, OW_ERR_INVALID for a value out of range (ow_runtime.hip)
struct QueryParams;
ow_status resolve_query_options(const ow_query_options *opts, QueryParams *qp);
// ow_buoyancy_options (NULL = defaults) -> the solver's settings and the model's constants (ow_runtime.hip)
struct BuoyancyParams;
ow_status resolve_buoyancy_options(const ow_buoyancy_options *opts, QueryParams *qp, BuoyancyParams *bp);
// ow_raycast_options (NULL = defaults) -> the ray cast's settings, OW_ERR_INVALID for a value out of range (ow_runtime.hip)
struct RaycastParams;
ow_status resolve_raycast_options(const ow_raycast_options *opts, RaycastParams *rp);
// the grow-only ray-cast scratch on the current device: `count` rays in, `count` records out, and the bound words (allocated once)
struct Ray;
struct RaycastHit;
ow_status raycast_scratch(int count, Ray **in, RaycastHit **out, int *capacity, uint32_t **bound);
// the host-side checks of ow_buoyancy / ow_group_buoyancy on host arrays: ranges, body indices, volumes, half heights (ow_runtime.hip)
ow_status check_buoyancy_arrays(const ow_buoyancy_body *bodies, int num_bodies, const ow_hull_point *hull, int num_points);
// The synchronous buoyancy's device half on `s` (ow_runtime.hip): grow-only scratch (*scratch, *scratch_bytes; on the current device), the
// arrays in, both kernels, the results (and, with points_inout, the records) out.  The caller synchronises.
struct DeviceBuffers;
struct SurfaceScales;
struct u16x4;
ow_status buoyancy_enqueue_host(int n, int cascades, const DeviceBuffers &buf, hipStream_t s, void **scratch, size_t *scratch_bytes,
                                const ow_buoyancy_body *bodies, int num_bodies, const ow_hull_point *hull, int num_points, const SurfaceScales &sc,
                                const QueryParams &qp, const BuoyancyParams &bp, ow_buoyancy_result *results, ow_buoyancy_point *points_inout,
                                const u16x4 *vel = nullptr);  // vel: the velocity layers (OW_BUOYANCY_WATER_VELOCITY)

}  // namespace ow

#define OW_HIP(call)                                                                                       \
    do {                                                                                                   \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess) return ow::fail(OW_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

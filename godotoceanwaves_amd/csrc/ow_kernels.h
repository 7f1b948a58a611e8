// ow_kernels.h -- internal launcher interface between the host units (ow_schedule.hip: the frame launchers; the read side's ow_*_host.hip and
// ow_group.hip: the consumer launchers) and the HIP translation units that hold the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "ow_device.h"
#include "ow_buoyancy.h"
#include "ow_environment.h"
#include "ow_raycast.h"
#include "ow_mesh.h"
#include "ow_mirror.h"
#include "ow_mist.h"
#include "ow_render.h"
#include "ow_rigid.h"
#include "ow_shadow.h"
#include "ow_sky_light.h"
#include "ow_solid.h"
#include "ow_solid_cast.h"
#include "ow_spray.h"
#include "ow_spray_draw.h"
#include "ow_surface.h"
#include "ow_velocity.h"
#include "ow_velocity_kernels.h"

namespace ow {

struct DeviceBuffers {
    cplx *h0;       // [layers][N][N] complex h0(k): first half of the `spectrum` texel (wave_generator.gd:31); the second half,
                    // conj(h0(-k)), is the mirrored texel of the same plane (Pass1::load_modulate)
    float *omega;   // [layers][N][N]          FP32 dispersion plane
    cplx *T;        // [launch slot][4 packed layers][N/16 y/16][N x'][16 y%16] complex: transposed intermediate (scratch between the
                    // two passes of ONE batch: indexed by the slot inside the launch, not by cascade, so every batch reuses it)
    u16x4 *disp;    // [layers][N][N] RGBA16F
    u16x4 *norm;    // [layers][N][N] RGBA16F (foam in .a)
    uint16_t *foam; // [layers][N x'][N/16 t][16 o] FP16: private copy of normal.a in pass-2 lane order (Pass2::foam_index)
    float *f32;     // [layers][N][N][8] or nullptr
    const cplx *tw; // twiddle table (plan_tw_total(N) entries)
    // compact-intermediate side buffers (Pass1::layer_input_c), scratch of one batch like T:
    cplx *pcol;     // [launch slot][N]     P(ky) of texel column id.x = 0, in pass-2 lane order (Pass2::pcol_index)
    cplx *rrow;     // [launch slot][N x'][4] row transforms Q1..Q3 of texel row id.y = 0 (entry 0 unused)
    const cplx *tw_split; // split plan (N = 2048): [twiddle table of the N/2 plan][W_N^k, k = 0 .. N/2 - 1]; nullptr otherwise
    const cplx *tw_half;  // half table (N = 2048, the compact pass 2: plan_twh_total(N) entries, ow_device.h "HALF TABLE"); nullptr otherwise
    uint32_t *status; // device status word (page-locked host memory, mapped): kernels OR kStatus* bits into it
};

// optional events bound to a launch's own dispatch packet (begin / end of the kernel itself)
struct LaunchTiming {
    hipEvent_t start = nullptr, stop = nullptr;
};

// The consumer launchers: called from the read side's ow_*_host.hip (for a context's own maps and, through its round trips, a group's gathered arrays).
// consumer-side sampling and the inverse query (ow_consumer.hip; per-point code and records in ow_surface.h)
hipError_t launch_sample_surface(int n, int cascades, const DeviceBuffers &buf, const float *xz_dev, int count,
                                 const SurfaceScales &scales, SurfaceSample *out_dev, hipStream_t s);
hipError_t launch_query_surface(int n, int cascades, const DeviceBuffers &buf, const float *xz_dev, int count, const SurfaceScales &scales,
                                const QueryParams &qp, SurfaceQuery *out_dev, hipStream_t s);
// buoyancy (ow_consumer.hip; per-point code, records and the summation order in ow_buoyancy.h): the per-point kernel over num_points hull
// points, then the per-body sums over num_bodies bodies, both on `s`.  pts_dev: the per-point records (read first with bp.warm_start).
hipError_t launch_buoyancy(int n, int cascades, const DeviceBuffers &buf, const BuoyancyBody *bodies_dev, int num_bodies, const HullPoint *hull_dev,
                           int num_points, const SurfaceScales &scales, const QueryParams &qp, const BuoyancyParams &bp, BuoyancyPoint *pts_dev,
                           BuoyancyResult *results_dev, hipStream_t s, const u16x4 *vel = nullptr);  // vel: the velocity layers (OW_BUOYANCY_WATER_VELOCITY)
// floating bodies (ow_consumer.hip; the state, the substep and its operation order in ow_rigid.h): the device arrays of one body set
struct BodiesArrays {
    RigidBody *state;        // [num_bodies]
    BuoyancyBody *records;   // [num_bodies] the pose records, formed from the states
    const HullPoint *hull;   // [num_points]
    BuoyancyPoint *pts;      // [num_points] per-point records: diagnostics and the warm start's state
    BuoyancyResult *results; // [num_bodies] of the last substep
    int32_t *flags;          // [num_bodies] 1: faulted (ow_rigid.h)
    int num_bodies, num_points;
};
// pose records, lowered flags and zeroed point records of bodies [first, first + count)
hipError_t launch_bodies_pose(const BodiesArrays &A, int first, int count, hipStream_t s);
// `substeps` substeps on `s`: fused, one k_bodies_step launch; otherwise substeps x (k_buoyancy_points[_moving], k_bodies_integrate).  The same bits.
hipError_t launch_bodies_step(int n, int cascades, const DeviceBuffers &buf, const BodiesArrays &A, const SurfaceScales &scales, const QueryParams &qp,
                              const BuoyancyParams &bp, const RigidParams &rp, int substeps, bool fused, hipStream_t s, const u16x4 *vel = nullptr);
// the velocity of the surface above each point (ow_consumer.hip; per-point code and the record in ow_velocity.h)
hipError_t launch_query_velocity(int n, int cascades, const DeviceBuffers &buf, const u16x4 *vel, const float *xz_dev, int count,
                                 const SurfaceScales &scales, const QueryParams &qp, SurfaceVelocity *out_dev, hipStream_t s);
// the velocity layers (ow_velocity.hip; kernels in ow_velocity_kernels.h): twiddle table tw (n entries exp(2 pi i m / n)) once, then per batch
// of args.count <= vel_batch(n) cascades pass 1 into `scratch` (args.count * vel_scratch_bytes(n)) and pass 2 into vel, both on `s`
hipError_t launch_velocity_twiddles(int n, cplx *tw, hipStream_t s);
hipError_t launch_velocity(int n, const VelocityArgs &args, const DeviceBuffers &buf, const cplx *tw, cplx *scratch, u16x4 *vel, hipStream_t s);
// ray casts (ow_consumer.hip; the rounds, records and the slab in ow_raycast.h): bound_dev (cascades words) is cleared, k_height_bound
// fills it, then k_raycast_surface casts `count` rays, all on `s`
hipError_t launch_raycast(int n, int cascades, const DeviceBuffers &buf, const Ray *rays_dev, int count, const SurfaceScales &scales,
                          const RaycastParams &rp, uint32_t *bound_dev, RaycastHit *out_dev, hipStream_t s);
// a camera view (ow_consumer.hip; the pixel rays, the march, the record and the composite in ow_render.h, the shading in ow_shading.h):
// bound_dev as for launch_raycast, then k_render_view writes cam.width x cam.height RGBA8 words and / or records (either may be null)
hipError_t launch_render_view(int n, int cascades, const DeviceBuffers &buf, const CameraParams &cam, const SurfaceScales &scales,
                              const RaycastParams &rp, const ShadeParams &sp, uint32_t *bound_dev, uint32_t *rgba_dev, RenderPixel *pixels_dev,
                              hipStream_t s);
// a mesh draw (ow_mesh.hip; the vertex stage, the coverage rule and the per-pixel record in ow_mesh.h).  MeshArrays: a mesh's device block.
struct MeshArrays {
    const float *local;      // [num_vertices][3] as uploaded
    const int32_t *indices;  // [num_triangles][3]
    MeshVertex *verts;       // [num_vertices] the resident vertex records of the last displace / draw
    uint32_t *counters;      // [4] triangles of the last draw by class (kTriSkipped .. kTriWave)
    int num_vertices, num_triangles;
};
// k_mesh_vertices alone: the records of M.verts (view positions only with a camera)
hipError_t launch_mesh_vertices(int n, int cascades, const DeviceBuffers &buf, const MeshArrays &M, const SurfaceScales &scales, const MeshParams &mp,
                                const CameraParams &cam, bool has_camera, const float origin[3], hipStream_t s);
// the whole draw: vertices, the clear of vis_dev (cam.width x cam.height words) and of the counters, raster, shade into RGBA8 words and / or
// records (either may be null), all on `s`
hipError_t launch_mesh_draw(int n, int cascades, const DeviceBuffers &buf, const MeshArrays &M, const SurfaceScales &scales, const MeshParams &mp,
                            const CameraParams &cam, const ShadeParams &sp, const float origin[3], uint64_t *vis_dev, uint32_t *rgba_dev,
                            RenderPixel *pixels_dev, hipStream_t s);
// a sea-spray step (ow_spray.hip; the schedule, start(), process() and the records in ow_spray.h).  SprayArrays: an emitter's device block.
struct SprayArrays {
    SprayParticle *particles;  // [amount]
    SprayInstance *instances;  // [amount]
    uint32_t *draw_list;       // [amount] the first *live_count entries: the live particles' indices, ascending
    uint32_t *block_words;     // [blocks][kSprayBlockWords] of the last step
    uint32_t *live_count;      // [1]
    uint64_t *totals;          // [2] particles :89 has spawned and rejected since creation
};
// k_spray_step, then k_spray_compact, both on `s`
hipError_t launch_spray_step(int n, int cascades, const DeviceBuffers &buf, const SprayArrays &A, const SurfaceScales &scales, const SprayParams &P,
                             const SprayClock &K, hipStream_t s);

// a billboard draw (ow_spray_draw.hip; the billboard, the coverage rule, fragment() and the blend in ow_spray_draw.h)
struct BillboardArrays {
    const SprayInstance *instances;  // [slots]
    const uint32_t *draw_list;       // [slots] or nullptr: slot k draws instance k
    const uint32_t *live_count;      // [1] or nullptr: every slot is live
    uint32_t slots;                  // an emitter's amount, or the caller's count
    SpraySprite *sprites;            // [slots] scratch
    uint32_t *counters;              // [2] billboards drawn and culled by the last draw; the masks lie behind them
    uint64_t *masks;                 // [ny][nx][words] scratch
    size_t clear_bytes;              // from counters to the end of the masks
};
// the clear of the counters and the masks, k_billboard_setup over A.slots slots, k_billboard_blend into the records (read and rewritten) and / or
// the RGBA8 words (either may be null), all on `s`
hipError_t launch_billboard_draw(const BillboardArrays &A, const CameraParams &cam, const SprayDrawParams &dp, const BillboardBins &bins, uint32_t *rgba_dev,
                                 RenderPixel *pixels_dev, hipStream_t s);

// a solid draw (ow_solid.hip; the vertex stage, the winner, the depth test and the shading in ow_solid.h, the coverage rule in ow_mesh.h)
struct SolidShape {          // an ow_solid's device arrays: what the draw and the shadow cast repeat per instance
    const float *local;      // [num_vertices][3] the shape, as uploaded
    const int32_t *indices;  // [num_triangles][3]
    int num_vertices, num_triangles;
};
struct SolidArrays {
    SolidShape shape;
    uint32_t *counters;      // [4] scratch: kSolidSkippedInstances .. kSolidWave of the last draw
    MeshVertex *verts;       // [instances][num_vertices] scratch
    uint64_t *vis;           // [cam.width x cam.height] scratch: the visibility words
};
// k_solid_clear, k_solid_vertices over in.count instances, k_solid_raster, k_solid_resolve into the records (read, rewritten where a solid is
// drawn) and / or the RGBA8 words (either may be null), all on `s`
hipError_t launch_solid_draw(const SolidArrays &A, const SolidInstances &in, const CameraParams &cam, const SolidParams &sp, uint32_t *rgba_dev,
                             RenderPixel *pixels_dev, hipStream_t s);

// a ray cast against solids (ow_solid_cast.hip; the intersection, the winner, the record and the bounding spheres in ow_solid_cast.h)
constexpr int kSolidCastSlots = 32;          // pairs of 64-bit sums a call's waves add into, by block index
constexpr int kSolidCastSlotWords = 16;      // 64-bit words from one pair to the next: 128 bytes
constexpr size_t kSolidCastSumsOffset = 128;  // the skipped instances (one 32-bit word) lie at 0
constexpr size_t kSolidCastCounterBytes = kSolidCastSumsOffset + (size_t)kSolidCastSlots * kSolidCastSlotWords * sizeof(uint64_t);
struct SolidCastArrays {
    SolidShape shape;
    const SolidCastBound *shape_bound;  // the shape's local sphere (launch_solid_cast_shape_bound wrote it)
    void *counters;                     // [kSolidCastCounterBytes] scratch: the counters of the last call
    SolidCastBound *bounds;             // [instances] scratch
};
// k_solid_cast_shape_bound: the shape's local centre and radius into *bound_dev, on `s`
hipError_t launch_solid_cast_shape_bound(const SolidShape &shape, SolidCastBound *bound_dev, hipStream_t s);
// the clear of the counters, k_solid_cast_bounds over in.count instances, k_solid_cast over `count` rays (water_dev: their water records, or
// null) into out_dev, all on `s`
hipError_t launch_solid_cast(const SolidCastArrays &A, const SolidInstances &in, const SolidCastParams &cp, const Ray *rays_dev, const RaycastHit *water_dev,
                             int count, SolidHit *out_dev, hipStream_t s);
// k_solid_cast_bounds over in.count instances: their world spheres into bounds_dev, the skipped ones added to *skipped_dev, on `s` (the
// mirror pass takes its spheres from here as well)
hipError_t launch_solid_cast_bounds(const SolidInstances &in, const SolidCastBound *shape_bound, SolidCastBound *bounds_dev, uint32_t *skipped_dev, hipStream_t s);

// the floating bodies' reflections (ow_mirror.hip; the arithmetic in ow_mirror.h).  The counters of a pass lie at the head of its scratch as
// a ray cast's do: the skipped instances (one 32-bit word) at 0, then kMirrorSlots copies of the kMirrorCounters 64-bit sums, a line each.
constexpr int kMirrorSlots = 32;
constexpr int kMirrorSlotWords = 16;
constexpr size_t kMirrorSumsOffset = 128;
constexpr size_t kMirrorCounterBytes = kMirrorSumsOffset + (size_t)kMirrorSlots * kMirrorSlotWords * sizeof(uint64_t);
struct MirrorArrays {
    SolidShape shape;                   // zeros without a solid (no instances then)
    const SolidCastBound *shape_bound;  // the shape's local sphere (launch_solid_cast_shape_bound wrote it)
    void *counters;                     // [kMirrorCounterBytes] scratch: the counters of the last pass
    SolidCastBound *bounds;             // [instances] scratch
};
// The clear of the counters, k_solid_cast_bounds over in.count instances, then k_mirror_apply over cam.width x cam.height records, rewritten
// in place, and their hit records (hits_dev may be null), on `s`.
hipError_t launch_mirror_apply(const MirrorArrays &A, const SolidInstances &in, const CameraParams &cam, const SkyLightParams &lp, const MirrorParams &mp,
                               RenderPixel *pixels_dev, SolidHit *hits_dev, hipStream_t s);

// the environment pass and the present (ow_environment.hip; the sky, the fog, the resolve, the tonemap and the transfer curve in ow_environment.h)
// k_environment_apply over cam.width x cam.height records, rewritten in place, on `s`; nothing is launched for a camera that is not finite
hipError_t launch_environment_apply(const CameraParams &cam, const EnvParams &ep, RenderPixel *pixels_dev, hipStream_t s);
// k_present<pp.s> over out_width x out_height output pixels of (out_width pp.s) x (out_height pp.s) records, into RGBA8 words and / or float4
// linear pixels (either may be null), on `s`
hipError_t launch_present(int out_width, int out_height, const PresentParams &pp, const RenderPixel *pixels_dev, uint32_t *rgba_dev, float *linear_dev,
                          hipStream_t s);

// light from the sky (ow_sky_light.hip; the pyramid's and the pass's arithmetic in ow_sky_light.h)
// k_radiance_decode, k_radiance_box down the sizes, k_radiance_prefilter per level from 1 on and k_radiance_irradiance, all on `s`
hipError_t launch_radiance_build(const RadianceBuild &b, hipStream_t s);
// k_sky_light_apply over cam.width x cam.height records, rewritten in place, on `s`; nothing is launched for a camera that is not finite
hipError_t launch_sky_light_apply(const CameraParams &cam, const SkyLightParams &lp, RenderPixel *pixels_dev, hipStream_t s);

// the sun shadows (ow_shadow.hip; the frame, the coverage rule, the filter and the record's arithmetic in ow_shadow.h)
struct ShadowArrays {
    SolidShape shape;        // the casting shape
    uint32_t *counters;      // [4] kShadowSkippedInstances .. kShadowWave since the last clear
    ShadowVertex *verts;     // [instances][num_vertices] scratch
    uint32_t *map;           // [size][size] the depth words
};
// k_shadow_clear over the map's size x size words and the counters, on `s`
hipError_t launch_shadow_clear(const ShadowArrays &A, int size, hipStream_t s);
// k_shadow_vertices over in.count instances, then k_shadow_raster, on `s`; nothing is launched without a frame (P.ok == 0) or instances
hipError_t launch_shadow_cast(const ShadowArrays &A, const SolidInstances &in, const ShadowParams &P, hipStream_t s);
// k_shadow_apply over cam.width x cam.height records, receivers rewritten in place, and the RGBA8 words (may be null), on `s`
hipError_t launch_shadow_apply(const uint32_t *map, const CameraParams &cam, const ShadowParams &P, const ShadowApply &ap, RenderPixel *pixels_dev,
                               uint32_t *rgba_dev, hipStream_t s);

// the height mist (ow_mist.hip; the medium, the slices, the depth compare and the pixel's arithmetic in ow_mist.h)
// The pass's kMistCounters counters cleared, then k_mist_apply over cam.width x cam.height records, rewritten in place, and the RGBA8 words
// (may be null), on `s`.  map: a shadow map's depth words, or null (no map, or one without a frame: P is not read then).
hipError_t launch_mist_apply(const uint32_t *map, const CameraParams &cam, const ShadowParams &P, const MistParams &mp, RenderPixel *pixels_dev, uint32_t *rgba_dev,
                             unsigned long long *counters_dev, hipStream_t s);

bool supported_map_size(int n);
int kernel_family(int n, int slots, int mode);  // 1 standard, 2 layer-parallel, 3 compact: what launch_pass1/2 will use
hipError_t launch_spectrum(int n, int cascade, const SpectrumPC &pc, const DeviceBuffers &buf, hipStream_t s);
hipError_t launch_pass1(int n, int slots, int mode, const FrameArgs &args, const DeviceBuffers &buf, hipStream_t s,
                        const LaunchTiming &lt = LaunchTiming{});  // mode: 0 auto, 1 standard, 2 layer-parallel, 3 compact
hipError_t launch_pass2(int n, int slots, int mode, const FrameArgs &args, const DeviceBuffers &buf, hipStream_t s,
                        const LaunchTiming &lt = LaunchTiming{});

// Tick groups for ow_run on small batches (ow_frame_kernels.h k_tick_group_c_lp): pass 2 of g.d2 consecutive ticks (scratch slots
// g.tbase2[j] + i) and / or pass 1 of g.d1 later ticks (times g.time1[j][i], scratch slots g.tbase1[j] + i) in one launch; n2 / n1 are
// filled in by the launcher.
bool tick_groups_supported(int n);
bool tick_pairs_supported(int n);
int tick_group_pipe_blocks(int n, int slots);  // pass-2 blocks of the pipelined form (0: not available at this map size)
hipError_t launch_tick_group(int n, const FrameArgs &args, const TickGroupArgs &g, const DeviceBuffers &buf, hipStream_t s,
                             const LaunchTiming &lt = LaunchTiming{}, hipStream_t side = nullptr);
// TWO CHAINS (round 6).  A tick-pair launch of four 1024^2 cascades on either side is exactly two generations of blocks, and the kernel boundary between
// two such launches costs a tenth of them: the chip drains (the last 8 us run below half occupancy) and fills again.  Cascades are independent, so the
// launch can go out as two launches of TWO cascades each on two streams -- the first halves of both sides on `s`, the second halves on `side` -- each a
// chain of its own (a half's pass 2 needs nothing but that half's pass 1 of the launch before): one chain's drain runs under the other's body.
// Same kernel, same items, same bits.  1024^2 x 4: 52.1 -> 48.0 us per tick on one box (scripts/two_ctx.py; everything else that was tried -- halves of
// other sizes, four chains, 2048^2 -- loses: a half must still fill the chip, and the two chains together must fit the Infinity Cache).
// tick_pair_splits: would launch_tick_group split this launch when given a side stream?  The caller orders the side stream (fork / join) around it.
bool tick_pair_splits(int n, const TickGroupArgs &g);

}  // namespace ow

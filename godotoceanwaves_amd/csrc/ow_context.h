// ow_context.h -- the context behind include/ocean_waves.h and the handles that hang off it, for the host units that work on them:
// ow_schedule.hip (the frame scheduler), ow_runtime.hip (create / destroy, status, scratch, hand-off, readback) and the read side's units
// (ow_consumer_host.h).  Every handle kind derives from ow::Handle and the context keeps ONE list of them: ow_consumer_host.hip holds their
// one life cycle, ow_destroy orphans whatever is still on the list.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ow_internal.h"

namespace ow {
// The FP32 time a record will be processed with `updates` updates from now: one FP64 add per update, in order (wave_generator.gd:103), narrowed
// last, by the pack (render_context.gd:131-134).
inline float time_after(double time, double delta, int updates) {
    for (int k = 0; k < updates; ++k) time += delta;
    return (float)time;
}
// Pass 1 of one cascade AS IT WAS COMPUTED ahead of time: all it depends on besides the layer's resident spectrum.
struct Pass1Key {
    int cascade = 0;
    float time = 0.0f, tile_x = 0.0f, tile_y = 0.0f;
    bool same_tiles(const ow_cascade_params &p) const { return p.tile_length[0] == tile_x && p.tile_length[1] == tile_y; }
    // is this what record p of `cascade` asks for `updates` updates of `delta` from now (0: as it is armed)?  FP32 times are compared bit for bit.
    bool serves(int for_cascade, const ow_cascade_params &p, double delta = 0.0, int updates = 0) const {
        const float t = time_after(p.time, delta, updates);
        return cascade == for_cascade && std::memcmp(&t, &time, 4) == 0 && same_tiles(p);
    }
};
inline Pass1Key pass1_key(int cascade, float time, const ow_cascade_params &p) { return Pass1Key{cascade, time, p.tile_length[0], p.tile_length[1]}; }

// What every device-resident handle of a context starts with.  No virtual destructor: the typed entry points delete their own type.
struct Handle {
    ow_context *ctx = nullptr;  // nullptr: orphaned by ow_destroy (the device block is gone, the handle is still the caller's to destroy)
    void *block = nullptr;      // the handle's one device allocation
};
}  // namespace ow

// a body set (ow_bodies_create): the block holds states, pose records, hull points, point records, results, fault flags
struct ow_bodies : ow::Handle {
    ow::BodiesArrays A{};
    int max_points = 0;     // the largest point_count of the set
    std::vector<int32_t> range;  // per body point_offset, point_count as created: ow_bodies_set_state may not change them
    uint64_t substeps = 0, fused_launches = 0, split_calls = 0;
};

// a mesh (ow_mesh_create): the block holds local positions, indices, vertex records, counters
struct ow_mesh : ow::Handle {
    ow::MeshArrays A{};
    uint64_t draws = 0;
};

// a sea-spray emitter (ow_spray_create): the block holds states, instances, draw list, per-block words, totals and live count
struct ow_spray : ow::Handle {
    ow::SprayArrays A{};
    ow::SprayParams P{};
    ow::SprayHostState H{};     // the FP64 clock and the host's bookkeeping
};

// a billboard material (ow_billboard_material_create): the block holds the sRGB table, the albedo texels, the dissolve texels
struct ow_billboard_material : ow::Handle {
    ow::SprayTexture albedo{}, dissolve{};
    const float *srgb = nullptr;
    float foam[3] = {0.0f, 0.0f, 0.0f}, max_alpha = 0.0f;
};

// a solid shape (ow_solid_create): the block holds local positions, indices and the shape's bounding sphere, which the first ray cast
// against the shape computes (ow_solid_cast.h)
struct ow_solid : ow::Handle {
    ow::SolidShape shape{};
    ow::SolidCastBound *bound = nullptr;
    bool bound_enqueued = false;  // k_solid_cast_shape_bound is on the context's stream, ahead of whatever reads *bound
};

// a panorama sky (ow_sky_create): the block holds the sRGB table and the texels
struct ow_sky : ow::Handle {
    ow::SprayTexture tex{};
    const float *srgb = nullptr;
    float energy = 1.0f;
};

// a radiance pyramid (ow_radiance_create): the block holds the levels, the irradiance, the unblurred chain and the host's tables
struct ow_radiance : ow::Handle {
    ow::RadiancePlan plan{};
    ow::RadianceLevel R[ow::kRadianceMaxLevels] = {};
    ow::RadianceLevel E{};
};

// a shadow map (ow_shadow_map_create): the block holds the counters and the depth words; the casters' vertex records (and uploaded
// transforms) lie in the map's own grow-only scratch, which goes with the map
struct ow_shadow_map : ow::Handle {
    int size = 0, device = 0;
    uint32_t *counters = nullptr, *map = nullptr;
    ow::ShadowParams P{};        // the frame of the last ow_shadow_map_begin (P.ok == 0: none yet)
    ow::DeviceScratch scratch;
    uint64_t casts = 0, instances_triangles = 0;  // since the last begin
};

struct ow_context {
    int n = 0, cascades = 0, layers = 0, device = 0;
    float depth = 20.0f;
    int kernel_mode = 0;  // 0 = by batch size, 1 = standard, 2 = layer-parallel, 3 = compact-intermediate kernels (OW_FLAG_KERNELS_*)
    int last_family = 0;  // kernel family of the most recent batch
    int bodies_mode = 0;  // ow_bodies_step: 0 = by the set's shape, 1 = fused, 2 = split (OW_FLAG_BODIES_*)
    hipStream_t stream = nullptr;
    bool own_stream = false, own_disp = false, own_norm = false;
    // TWO CHAINS (ow_kernels.h): tick-pair launches of four 1024^2 cascades a side go out as two launches of two cascades, the second halves on side_stream.
    // side_active: work of the second chain is in flight that `stream` has not been made to wait for -- since the fork NOTHING but first-chain launches has
    // been enqueued on `stream` (everything else goes through main_stream(), which joins first).
    hipStream_t side_stream = nullptr;
    hipEvent_t side_fork_ev = nullptr, side_join_ev = nullptr;
    bool side_active = false;
    uint64_t split_launches = 0;  // launches that went out as two chains (ow_chain_stats)
    ow::DeviceBuffers buf{};
    ow::cplx *tw_dev = nullptr, *tw_split_dev = nullptr, *tw_half_dev = nullptr;
    // generator state per invocation of update() (wave_generator.gd:13-15).  The reference keeps a reference to the caller's
    // Array; a C caller's memory is only borrowed for the duration of a call, so the context keeps COPIES of the armed records
    // (ow_set_cascade_params / ow_get_cascade_params are the explicit form of "the parameter objects are live")
    ow_cascade_params pass_parameters[OW_MAX_CASCADES] = {};
    int pass_count = 0;
    int pass_num_cascades_remaining = 0;
    // device status word: page-locked host memory mapped into the device; kernels OR error bits into it (a bounded
    // device-side spin that gave up), every synchronising entry point turns a non-zero word into OW_ERR_HIP
    uint32_t *status_host = nullptr;
    uint32_t inject_fault = 0;  // ow_debug_inject_fault: applied to the next batch only
    // The status word is consumed by the first synchronising call that sees it; the failure itself is sticky: until the next batch
    // is enqueued every call that hands out map bytes (ow_get_maps, ow_get_maps_f32, ow_sample_surface) keeps failing, and so does
    // the ow_readback_wait of every layer whose copy was in flight when the word was consumed (readback_faulted).
    // Both are bit masks over the array layers: a synchronising call that finds the word set marks the layers recomputed by the batches
    // enqueued since the previous synchronisation (enqueued_since_sync); a layer's mark is lifted only by a later batch that recomputes
    // THAT layer (the reference's schedule enqueues one cascade per call: the other layers keep the faulted batch's bytes).
    uint32_t maps_faulted = 0, enqueued_since_sync = 0;
    uint32_t readback_faulted = 0;
    ow_push_constants pc_words[OW_MAX_CASCADES] = {};  // what the reference would have packed for each cascade's most recent launch (ow_get_push_constants)
    bool pc_valid[OW_MAX_CASCADES] = {};
    // pc_words[i].spectrum are the constants layer i's RESIDENT spectrum (h0, omega) was generated from -- k_spectrum is a deterministic function
    // of those thirteen words and the map size, so a dirty record that packs to the same words is served by what is there (spectrum_is_resident)
    bool spectrum_resident[OW_MAX_CASCADES] = {};
    bool always_regenerate = false;  // OW_FLAG_ALWAYS_REGENERATE_SPECTRUM: every dirty flag launches k_spectrum, as the reference does
    uint64_t spectra_generated = 0, spectra_skipped = 0;  // ow_spectrum_stats
    // ow_update_all's adaptive look-ahead (lookahead_tick below): a pass 1 of the NEXT tick, speculated with the caller's last delta.
    // Invariant: queued > 0 exactly while the scratch holds pass 1 of `queued` ticks that nothing has disturbed since; whatever else
    // writes the scratch (or may have corrupted it) drops it (ow::drop_computed_ahead, ow_schedule.h), and no field below is read while it is 0.
    struct Lookahead {
        static constexpr int kMaxAhead = 4;  // ticks of pass 1 one launch may compute ahead (group kernel; the pair kernel takes one)
        int count = 0, mode = 0;       // cascades per tick; 1 = compact family (pair kernel), 2 = layer-parallel compact family (group kernel)
        int queued = 0, head = 0;      // ring of ticks computed ahead: entries head, head + 1, .. (mod kMaxAhead)
        int group[kMaxAhead] = {};     // scratch group (of `stride` launch slots) that holds each entry's intermediate
        ow::Pass1Key p1[kMaxAhead][OW_MAX_CASCADES] = {};  // what each entry holds, per launch slot of the launch that will use the entry
        int cur_group = 0;             // group that held the most recent launch's own intermediate
        double last_delta = -1.0;      // the previous ow_update's delta, and for how many calls in a row it has been the same
        double streak_delta = -1.0;    // ... "the same" = equal to the delta that STARTED the streak (a slowly ramping delta is not one unbroken streak)
        int streak = 0;
        int prev_run = 1;              // updates in the caller's previous run of equal deltas (1: none that says anything)
        uint64_t hits = 0, speculated = 0;
        bool hold = false;             // ow_run is about to merge the following ticks itself: its first tick must not speculate for them
        int certain = 0;               // ticks the caller GUARANTEES will follow with the same delta (ow_run's own remaining ticks): speculated without evidence
    } la;
    // ow_run after ow_run (run_impl): what the last launch of a run computed ahead for the first launch of the NEXT run like it
    struct RunAhead {
        bool armed = false;          // the scratch holds that pass 1 and nothing has disturbed it since
        int kind = 0;                // 1 = tick groups: pass 1 of `ticks` consecutive ticks of all `count` cascades; 2 = tick pairs: pass 1 of one batch, one tick
        int count = 0;               // cascades per tick of the run that computed it
        int D = 0, ticks = 0, pos = 0;  // kind 1: ticks per group of that run, ticks computed ahead, ring position (in ticks, mod 2 D) of the first of them
        int batch = 0, first = 0, size = 0, parity = 0;  // kind 2: the batch (its first launch slot, its cascades) and the half of the scratch its intermediate is in
        ow::Pass1Key p1[ow::kMaxTickGroup][OW_MAX_CASCADES] = {};  // what it holds, per tick (kind 2: entry 0) and launch slot; kind 2 keeps the tile lengths of
                                                                // the other batches' slots there too (the run checks them: run_resume_usable)
        bool last_was_run = false;   // the most recent tick-advancing call was an ow_run (lowered by ow_update / ow_update_all / ow_process from outside a run)
        int last_count = 0;
        double last_delta = 0.0;
        int run_streak = 0;          // how many runs like this one (same delta, same count) have preceded it without anything in between
    } ra;
    bool inside_run = false;    // ow_run is executing (its own ow_update_all calls are not "something in between")
    int run_frames = 0;         // ... with this many ticks (may_split)
    int pair_dir = 0;           // direction of the next block of the cascade-major pair stream (batches 0 .. B-1 or B-1 .. 0): alternates, across runs too
    bool run_as_calls = false;  // OW_FLAG_RUN_AS_CALLS
    bool run_as_reference = false;  // OW_FLAG_RUN_AS_REFERENCE_SCHEDULE
    bool no_merge = false;      // OW_FLAG_NO_TICK_GROUPS
    int group_depth_forced = 0;  // OW_DEBUG_TICK_GROUP_DEPTH (measurements; read once)
    int run_delta_period = 0;    // OW_DEBUG_RUN_DELTA_CHANGE_EVERY: the call-by-call forms of ow_run (OW_FLAG_RUN_AS_CALLS / _AS_REFERENCE_SCHEDULE) switch
                                 // between delta and 1.25 delta every that many ticks -- an irregular caller for the look-ahead to miss on (measurements)
    int ahead_depth = 0;      // ticks of pass 1 ow_update_all's look-ahead computes per launch once the deltas keep repeating (OW_DEBUG_LOOKAHEAD_DEPTH, read once)
    int pair_tick_block = 0;  // ticks a batch runs through before the stream of tick pairs moves on to the next batch (0: by map size; OW_DEBUG_PAIR_TICK_BLOCK, read once)
    size_t pair_texels = 0;  // batch size of ow_run's tick pairs, in texels (kPairTexels; OW_DEBUG_PAIR_TEXELS is read ONCE, by ow_create)
    // ow_run's tick groups (k_tick_group_c_lp): the largest cascade count they serve (0 = not available) and how many ticks go
    // into one group; the scratch buffers hold 2 * depth * count cascades then
    int group_p1_form = -1, group_p2_form = -1;
    int group_max_count = 0, group_depth = 0;  // (group_depth: the depth of a run of group_max_count cascades; a run's own depth follows its count)
    int scratch_slots = 0;  // launch slots the scratch intermediate (T, pcol, rrow) holds now: one batch at create, grown by the first ow_run that merges launches
    // ow_run's tick pairs on the compact family (k_tick_pair_c): the largest batch they launch (0 = never); scratch two batches deep
    int pair_slots = 0;
    int last_group_depth = 0;  // ticks per launch of the most recent ow_run that went out in groups / pairs
    // timing: a pool of events so that timed ticks stay enqueued back to back
    int timing = 0;  // 0 off, 1 per pass (ow_run stays on one launch per pass), 2 as launched (tick groups / pairs stay on, timed per launch)
    std::vector<char> ev_single;  // per 4-event record: 1 = one launch (events 0, 1 only): a tick group / pair
    std::vector<hipEvent_t> ev;  // 4 per timed batch: start/stop of the pass-1 dispatch, start/stop of the pass-2 dispatch
    size_t ev_used = 0;
    double t1_ms = 0, t2_ms = 0, tg_ms = 0;
    int t_launches = 0, tg_launches = 0;
    int slot_of[OW_MAX_CASCADES];  // launch slot of each cascade in the most recent batch, -1 if it was not in it
    // last batch that was launched (for ow_probe_kernel_times)
    ow::FrameArgs last_args{};
    int last_count = 0;
    // hand-off to a host consumer (ow_readback_*): device snapshot + page-locked staging, one slot per layer and map
    hipStream_t copy_stream = nullptr;
    ow::u16x4 *snap_dev = nullptr, *snap_host = nullptr;  // [2 maps][layers][N][N]
    hipEvent_t snap_ready[OW_MAX_CASCADES] = {}, copy_done[OW_MAX_CASCADES] = {};
    bool copy_pending[OW_MAX_CASCADES] = {};
    // The consumers' grow-only scratch (the read side's ow_*_host.hip).  query: the synchronous point calls' points in and records out (of the largest kind);
    // buoy: bodies, hull points, per-point records, results; ray: rays in, records out; render_rgba / render_pixels: the RGBA8 words and per-pixel
    // records of the synchronous ow_render_view, ow_mesh_draw and ow_billboard_draw; mesh_vis: the draw's visibility words (both forms);
    // billboard: a billboard draw's counters, bin masks, sprite records and (ow_billboard_draw_instances) the uploaded instances;
    // solid: a solid draw's counters, transformed vertex records, visibility words and (ow_solid_draw_instances) the uploaded transforms.
    // solid_cast: a ray cast's counters and instance spheres, the uploaded transforms (ow_cast_instances) and, in the synchronous
    // forms, the rays, the water records and the hit records.
    // The synchronous ow_shadow_apply uses render_pixels and render_rgba; a shadow map's scratch is the map's own (ow_shadow_map).
    // The synchronous ow_environment_apply uses render_pixels; the synchronous ow_present render_pixels for the records and render_rgba for both
    // outputs (the float4 pixels first, then the RGBA8 words).  Their asynchronous forms use no scratch.
    // mist: the copies of the three 64-bit counters of the last ow_mist_apply (ow_mist.h kMistCounterBytes), allocated by the first pass in either form;
    // the synchronous form uses render_pixels and render_rgba as well.
    // mirror: the counters of the last ow_mirror_apply and its instance spheres, the uploaded transforms (ow_mirror_apply_instances) and, in the
    // synchronous forms, the hit records; those forms use render_pixels as well.
    ow::DeviceScratch query_scratch, buoy_scratch, ray_scratch, render_rgba, render_pixels, mesh_vis, billboard, solid, solid_cast, mist, mirror;
    uint64_t mirror_passes = 0;    // ow_mirror_stats
    uint64_t mist_passes = 0;      // ow_mist_stats
    uint64_t billboard_draws = 0;  // ow_billboard_draw_stats
    uint64_t solid_draws = 0;      // ow_solid_draw_stats
    uint64_t solid_casts = 0;      // ow_cast_stats
    uint32_t *ray_bound = nullptr;  // the per-cascade bound words of the slab (ray casts and views), allocated once
    // the velocity layers (ow_update_velocity; ow_velocity_kernels.h): V in the displacement array's layout, the pipeline's own intermediate
    // (vel_slots cascades of one launch pair) and twiddle table, all allocated by the first velocity call
    ow::u16x4 *vel = nullptr;
    ow::cplx *vel_scratch = nullptr, *vel_tw = nullptr;
    int vel_slots = 0;
    // Layers whose V no longer belongs to their maps: set by mark_recomputed (every batch that recomputes a layer), cleared by the velocity
    // launch that computes them.  spectrum_ahead: layers whose resident spectrum was regenerated by a batch that did not get as far as
    // launching their pass 2 (enqueue); their h0 is newer than their maps, and their velocity is refused until a batch recomputes them.
    uint32_t velocity_stale = 0, spectrum_ahead = 0;
    uint64_t vel_computed = 0, vel_skipped = 0;  // ow_velocity_stats
    std::vector<ow::Handle *> handles;  // the live handles of this context, of every kind: ow_destroy orphans what the caller has not destroyed
    uint64_t host_syncs = 0;  // stream synchronisations made on the caller's thread since ow_create (ow_sync_stats)
};

// The services of the frame side the read side needs (main_stream: ow_schedule.hip, the others: ow_runtime.hip).
namespace ow {
// The stream everything but a first-chain launch is enqueued on or synchronised through: joins the second chain first (a no-op when none is in flight).
hipStream_t main_stream(ow_context *c);
// hipStreamSynchronize + the device status word.  layer_mask: the array layers whose bytes the caller is about to hand to ITS caller (0 for a
// bare ow_sync), refused while they are those of a faulted batch.
ow_status sync_stream(ow_context *c, uint32_t layer_mask);
ow_status refuse_faulted(const ow_context *c, uint32_t layer_mask);
ow_status check_cascade(const ow_context *c, int cascade);
inline size_t plane(const ow_context *c) { return (size_t)c->n * c->n; }
// array layers [0, num_cascades) as a bit mask
inline uint32_t layer_mask(int num_cascades) { return (1u << num_cascades) - 1u; }
}  // namespace ow

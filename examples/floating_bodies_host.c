/* floating_bodies_host.c -- a few hundred crates of different sizes floating on the generator's maps, from plain C99: the bodies, their
 * hulls and their states live on the device.  The crates are launched at the height of the water above them; then every frame advances the
 * three cascades of the demo scene (ow_update_all) and enqueues ONE ow_bodies_step of 4 substeps behind it, with the drag taken against the
 * moving water (OW_BUOYANCY_WATER_VELOCITY).  The context runs on a stream of this program's, so every fourth frame it also enqueues, in
 * stream order, two device-to-device copies of the set's pose and result records (ow_bodies_get_device_ptrs) into a history buffer: what
 * a renderer's instance-buffer update would be.  Nothing is synchronised and nothing crosses the bus inside the loop (ow_sync_stats is read
 * before and after it); states and history are read back once, at the end.  (examples/buoyancy_host.c is the same physics with the
 * integrator on the host: one round trip per substep.)
 *   gcc -O2 -std=c99 -Iinclude examples/floating_bodies_host.c -o floating_bodies_host -Lgodotoceanwaves_amd -locean_waves \
 *       -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/godotoceanwaves_amd -Wl,-rpath,/opt/rocm/lib -lm && ./floating_bodies_host [frames]
 * Prints key=value pairs.  afloat is buoyancy_host.c's criterion PER CRATE over the history: everything finite, the crate's mean submerged
 * share over time between a fifth and four fifths (share_min / share_max: the smallest and largest of the 256 means), and its origin
 * within 5 m of the water.  buoyancy_host.c measures those 5 m from the mean level, which holds for one box at one place over a few
 * seconds; over this field the water itself leaves that band (water_min / water_max: the surface sampled every 3 m over the field at the
 * end; y_min / y_max: the crates' heights over the whole history), so here they are measured from the water above each crate at the end
 * (ow_query_surface; off_water_max is the largest distance).  Also: the bodies the device flagged as faulted and host_syncs, the stream
 * synchronisations the library made inside the loop (0). */
#include "scene.h"

#define CRATES 256
#define NX 3
#define NY 4
#define NZ 3
#define PER_CRATE (NX * NY * NZ)

static ow_rigid_body bodies[CRATES];
static ow_hull_point hull[CRATES * PER_CRATE];
static ow_buoyancy_result results[CRATES];
static ow_buoyancy_body bodies_rec[CRATES];
static double volume_of[CRATES];
static float crate_xz[CRATES][2];
static ow_surface_query water[CRATES];
#define GRID 64
static float grid_xz[GRID * GRID][2];
static ow_surface_query grid_water[GRID * GRID];
#define SNAP_EVERY 4

int main(int argc, char **argv) {
    const int frames = scene_arg(argc, argv, 1, 300), substeps = 4;
    const int n = 256, cascades = SCENE_CASCADES;
    const double frame_dt = 1.0 / 60.0, rho = 1025.0;
    const int snaps = frames / SNAP_EVERY;
    int status = 1;
    uint64_t syncs_before = 0, syncs_after = 0;
    void *stream = NULL, *bodies_dev = NULL, *results_dev = NULL, *hist_bodies = NULL, *hist_results = NULL;
    ow_buoyancy_body *hb = NULL;
    ow_buoyancy_result *hr = NULL;
    ow_context *ctx = NULL;
    ow_bodies *set = NULL;
    if (snaps < 1) { fprintf(stderr, "at least %d frames\n", SNAP_EVERY); return 1; }
    if (hipStreamCreate(&stream)) { fprintf(stderr, "hipStreamCreate failed (this library has no CPU fallback)\n"); return 1; }

    ow_config cfg;
    scene_config(&cfg, n);
    cfg.stream = stream;
    if (ow_create(&cfg, &ctx) != OW_OK) { fprintf(stderr, "ow_create: %s\n", ow_last_error()); (void)hipStreamDestroy(stream); return 1; }

    ow_cascade_params par[SCENE_CASCADES];
    float map_scales[SCENE_CASCADES][4];
    scene_cascades(par, map_scales);

    /* the crates: a 16 x 16 grid 12 m apart, sizes from 1 to 3 m, each of half the water's density, voxelised into NX x NY x NZ points */
    memset(bodies, 0, sizeof bodies);
    memset(hull, 0, sizeof hull);
    for (int b = 0; b < CRATES; ++b) {
        const double size[3] = {1.0 + (b % 5) * 0.5, 0.8 + (b % 3) * 0.4, 1.0 + (b % 7) * 0.3};
        const double volume = size[0] * size[1] * size[2], mass = 0.5 * rho * volume;
        ow_rigid_body *B = &bodies[b];
        volume_of[b] = volume;
        B->position[0] = (b % 16 - 7.5) * 12.0; B->position[1] = 0.0; B->position[2] = (b / 16 - 7.5) * 12.0;
        B->orientation[3] = 1.0;
        B->mass = mass;
        B->inverse_inertia[0] = 12.0 / (mass * (size[1] * size[1] + size[2] * size[2]));
        B->inverse_inertia[1] = 12.0 / (mass * (size[0] * size[0] + size[2] * size[2]));
        B->inverse_inertia[2] = 12.0 / (mass * (size[0] * size[0] + size[1] * size[1]));
        B->linear_drag = 3.0f; B->quadratic_drag = 0.5f;
        B->point_offset = b * PER_CRATE; B->point_count = PER_CRATE;
        for (int i = 0, k = b * PER_CRATE; i < NX; ++i)
            for (int j = 0; j < NY; ++j)
                for (int l = 0; l < NZ; ++l, ++k) {
                    hull[k].local[0] = (float)((i + 0.5) * size[0] / NX - size[0] / 2);
                    hull[k].local[1] = (float)((j + 0.5) * size[1] / NY - size[1] / 2);
                    hull[k].local[2] = (float)((l + 0.5) * size[2] / NZ - size[2] / 2);
                    hull[k].volume = (float)(volume / PER_CRATE);
                    hull[k].half_height = (float)(size[1] / NY / 2);
                    hull[k].body = b;
                }
    }
    /* launch the crates from the water: the maps of the first tick, the height above each crate (both before the loop) */
    if (ow_update_all(ctx, frame_dt, par, cascades) != OW_OK) goto fail;
    for (int b = 0; b < CRATES; ++b) {
        crate_xz[b][0] = (float)bodies[b].position[0];
        crate_xz[b][1] = (float)bodies[b].position[2];
    }
    if (ow_query_surface(ctx, &crate_xz[0][0], CRATES, &map_scales[0][0], cascades, NULL, water) != OW_OK) goto fail;
    for (int b = 0; b < CRATES; ++b) bodies[b].position[1] = (double)water[b].height;
    if (ow_bodies_create(ctx, bodies, CRATES, hull, CRATES * PER_CRATE, &set) != OW_OK) goto fail;

    if (ow_bodies_get_device_ptrs(ctx, set, &bodies_dev, &results_dev, NULL) != OW_OK) goto fail;
    if (hipMalloc(&hist_bodies, (size_t)snaps * sizeof bodies_rec) || hipMalloc(&hist_results, (size_t)snaps * sizeof results)) {
        fprintf(stderr, "hipMalloc failed\n");
        goto out;
    }

    ow_bodies_options opts;
    memset(&opts, 0, sizeof opts);
    /* density 1025, gravity 9.81, water level 0: the defaults.  The drag is taken against the MOVING water: this sea heaves faster than a
     * crate dragged against still water can rise (g / (2 k_lin) = 1.6 m/s), which would hold the small crates under the crests. */
    opts.buoyancy.flags = OW_BUOYANCY_WARM_START | OW_BUOYANCY_WATER_VELOCITY;

    if (ow_sync_stats(ctx, &syncs_before) != OW_OK) goto fail;
    for (int frame = 0; frame < frames; ++frame) {   /* enqueues only: no synchronisation, nothing to or from the host */
        if (ow_update_all(ctx, frame_dt, par, cascades) != OW_OK) goto fail;
        if (ow_bodies_step(ctx, set, &map_scales[0][0], cascades, &opts, substeps, frame_dt / substeps) != OW_OK) goto fail;
        if (frame % SNAP_EVERY == SNAP_EVERY - 1 && frame / SNAP_EVERY < snaps) {   /* the caller's own work, ordered by the stream alone */
            const size_t k = (size_t)(frame / SNAP_EVERY);
            if (hipMemcpyAsync((char *)hist_bodies + k * sizeof bodies_rec, bodies_dev, sizeof bodies_rec, HIP_DEVICE_TO_DEVICE, stream) ||
                hipMemcpyAsync((char *)hist_results + k * sizeof results, results_dev, sizeof results, HIP_DEVICE_TO_DEVICE, stream)) {
                fprintf(stderr, "hipMemcpyAsync failed\n");
                goto out;
            }
        }
    }
    if (ow_sync_stats(ctx, &syncs_after) != OW_OK) goto fail;

    {
        uint64_t taken = 0, fused = 0, split = 0, faulted = 0;
        int finite = 1, afloat = 1;
        double share = 0.0, y_min = 1e30, y_max = -1e30, share_min = 1e30, share_max = -1e30, water_min = 1e30, water_max = -1e30, off_max = 0.0;
        if (ow_bodies_get_state(ctx, set, 0, CRATES, bodies) != OW_OK) goto fail;   /* synchronises: after the loop */
        if (ow_bodies_get_results(ctx, set, 0, CRATES, results) != OW_OK) goto fail;
        if (ow_bodies_stats(ctx, set, &taken, &fused, &split, &faulted) != OW_OK) goto fail;
        hb = (ow_buoyancy_body *)malloc((size_t)snaps * sizeof bodies_rec);
        hr = (ow_buoyancy_result *)malloc((size_t)snaps * sizeof results);
        if (!hb || !hr || hipMemcpy(hb, hist_bodies, (size_t)snaps * sizeof bodies_rec, HIP_DEVICE_TO_HOST) ||
            hipMemcpy(hr, hist_results, (size_t)snaps * sizeof results, HIP_DEVICE_TO_HOST)) {
            fprintf(stderr, "history read-back failed\n");
            goto out;
        }
        for (int b = 0; b < CRATES; ++b) {
            crate_xz[b][0] = (float)bodies[b].position[0];
            crate_xz[b][1] = (float)bodies[b].position[2];
        }
        if (ow_query_surface(ctx, &crate_xz[0][0], CRATES, &map_scales[0][0], cascades, NULL, water) != OW_OK) goto fail;
        for (int i = 0; i < GRID * GRID; ++i) {   /* the surface itself, every 3 m over the field */
            grid_xz[i][0] = (float)((i % GRID - GRID / 2) * 3.0);
            grid_xz[i][1] = (float)((i / GRID - GRID / 2) * 3.0);
        }
        if (ow_query_surface(ctx, &grid_xz[0][0], GRID * GRID, &map_scales[0][0], cascades, NULL, grid_water) != OW_OK) goto fail;
        for (int i = 0; i < GRID * GRID; ++i) {
            if (grid_water[i].height < water_min) water_min = grid_water[i].height;
            if (grid_water[i].height > water_max) water_max = grid_water[i].height;
        }
        for (int b = 0; b < CRATES; ++b) {
            const ow_rigid_body *B = &bodies[b];
            const double off = fabs(B->position[1] - (double)water[b].height);
            double s = 0.0;
            int ok = 1;
            for (int i = 0; i < 3; ++i)
                ok &= isfinite(B->position[i]) && isfinite(B->linear_velocity[i]) && isfinite(B->angular_velocity[i]) && isfinite(results[b].force[i]) &&
                      isfinite(results[b].torque[i]);
            for (int i = 0; i < 4; ++i) ok &= isfinite(B->orientation[i]);
            for (int k = 0; k < snaps; ++k) {   /* the crate over time */
                const double y = hb[(size_t)k * CRATES + b].transform[10];
                ok &= isfinite(y) && isfinite(hr[(size_t)k * CRATES + b].submerged_volume);
                s += hr[(size_t)k * CRATES + b].submerged_volume / volume_of[b] / snaps;
                if (y < y_min) y_min = y;
                if (y > y_max) y_max = y;
            }
            finite &= ok;
            afloat &= ok && s > 0.2 && s < 0.8 && off < 5.0;
            share += s / CRATES;
            if (s < share_min) share_min = s;
            if (s > share_max) share_max = s;
            if (off > off_max) off_max = off;
        }
        printf("bodies=%d frames=%d substeps=%llu fused_launches=%llu split_calls=%llu faulted=%llu snapshots=%d submerged_share=%.4f share_min=%.4f "
               "share_max=%.4f off_water_max=%.4f y_min=%.4f y_max=%.4f water_min=%.4f water_max=%.4f finite=%d afloat=%d host_syncs=%llu\n", CRATES,
               frames, (unsigned long long)taken, (unsigned long long)fused, (unsigned long long)split, (unsigned long long)faulted, snaps, share,
               share_min, share_max, off_max, y_min, y_max, water_min, water_max, finite, afloat, (unsigned long long)(syncs_after - syncs_before));
    }
    status = 0;
    goto out;
fail:
    fprintf(stderr, "ocean_waves: %s\n", ow_last_error());
out:
    free(hb); free(hr);
    (void)hipFree(hist_bodies); (void)hipFree(hist_results);
    ow_bodies_destroy(ctx, set);
    ow_destroy(ctx);
    (void)hipStreamDestroy(stream);
    return status;
}

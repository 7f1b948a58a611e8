/* spray_host.c -- the reference scene's sea-spray emitter from plain C99: creates a context over the three cascades, creates the
 * WaterSprayEmitter of main.tscn:133-140 (ow_spray_options_default), and for a few seconds of the scene's update delta ticks the waves
 * and steps the emitter behind them in the context's stream order, printing the live count of every step.
 *   gcc -O2 -std=c99 -Iinclude examples/spray_host.c -o spray_host -Lgodotoceanwaves_amd -locean_waves \
 *       -Wl,-rpath,$PWD/godotoceanwaves_amd -Wl,-rpath-link,/opt/rocm/lib -lm && ./spray_host [steps [map_size [amount]]]
 * The scene is mesh_host.c's.  Prints one "step=K live=N" line per step, then key=value pairs: the emitter's clock, the restarts the
 * schedule made, the particles the spawn decision (sea_spray_particle.gdshader:89) let through and rejected, and whether every instance
 * of the last step is finite. */
#include "scene.h"

int main(int argc, char **argv) {
    const int steps = scene_arg(argc, argv, 1, 150), n = scene_arg(argc, argv, 2, 256), cascades = SCENE_CASCADES;
    const double dt = 1.0 / 50.0;   /* water.gd:51 */
    int status = 1;

    ow_config cfg;
    scene_config(&cfg, n);
    ow_context *ctx = NULL;
    ow_spray *spray = NULL;
    ow_spray_instance *inst = NULL;
    uint32_t *draw = NULL;
    if (ow_create(&cfg, &ctx) != OW_OK) { fprintf(stderr, "ow_create: %s\n", ow_last_error()); return 1; }

    ow_cascade_params par[SCENE_CASCADES];
    float map_scales[SCENE_CASCADES][4];
    scene_cascades(par, map_scales);

    ow_spray_options opts;
    ow_spray_options_default(&opts);   /* mat_spray.tres, main.tscn:133-140 */
    if (argc > 3) opts.amount = (uint32_t)atoi(argv[3]);
    if (ow_spray_create(ctx, &opts, &spray) != OW_OK) goto fail;

    for (int k = 0; k < steps; ++k) {
        uint32_t live = 0;
        if (ow_update_all(ctx, dt, par, cascades) != OW_OK) goto fail;
        if (ow_spray_step(ctx, spray, dt, &map_scales[0][0], cascades) != OW_OK) goto fail;   /* enqueued behind the tick, no synchronisation */
        if (ow_spray_read(ctx, spray, NULL, NULL, NULL, &live) != OW_OK) goto fail;
        printf("step=%d live=%u\n", k, (unsigned)live);
    }

    {
        uint32_t live = 0;
        double time = 0.0;
        uint64_t taken = 0, restarts = 0, spawned = 0, rejected = 0;
        int finite = 1, ascending = 1;
        inst = (ow_spray_instance *)malloc((size_t)opts.amount * sizeof(ow_spray_instance));
        draw = (uint32_t *)malloc((size_t)opts.amount * sizeof(uint32_t));
        if (!inst || !draw) { fprintf(stderr, "out of memory\n"); goto out; }
        if (ow_spray_read(ctx, spray, inst, NULL, draw, &live) != OW_OK) goto fail;
        if (ow_spray_stats(ctx, spray, &time, &taken, &restarts, &spawned, &rejected) != OW_OK) goto fail;
        for (uint32_t i = 0; i < opts.amount; ++i) {
            for (int k = 0; k < 12; ++k) finite &= isfinite(inst[i].transform[k]) ? 1 : 0;
            for (int k = 0; k < 4; ++k) finite &= isfinite(inst[i].custom[k]) ? 1 : 0;
        }
        for (uint32_t k = 1; k < live; ++k) ascending &= draw[k - 1] < draw[k] ? 1 : 0;
        printf("amount=%u steps=%llu time=%.6f restarts=%llu spawned=%llu rejected=%llu live=%u ascending=%d finite=%d\n", (unsigned)opts.amount,
               (unsigned long long)taken, time, (unsigned long long)restarts, (unsigned long long)spawned, (unsigned long long)rejected, (unsigned)live,
               ascending, finite);
    }
    status = 0;
    goto out;
fail:
    fprintf(stderr, "ocean_waves: %s\n", ow_last_error());
out:
    free(inst); free(draw);
    ow_spray_destroy(ctx, spray);
    ow_destroy(ctx);
    return status;
}

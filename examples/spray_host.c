/* spray_host.c -- the reference scene's sea-spray emitter from plain C99: creates a context over the three cascades, creates the
 * WaterSprayEmitter of main.tscn:133-140 (ow_spray_options_default), and for a few seconds of the scene's update delta ticks the waves
 * and steps the emitter behind them in the context's stream order, printing the live count of every step.
 *   gcc -O2 -std=c99 -Iinclude examples/spray_host.c -o spray_host -Lgodotoceanwaves_amd -locean_waves \
 *       -Wl,-rpath,$PWD/godotoceanwaves_amd -Wl,-rpath-link,/opt/rocm/lib -lm && ./spray_host [steps [map_size [amount]]]
 * The scene is mesh_host.c's.  Prints one "step=K live=N" line per step, then key=value pairs: the emitter's clock, the restarts the
 * schedule made, the particles the spawn decision (sea_spray_particle.gdshader:89) let through and rejected, and whether every instance
 * of the last step is finite. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ocean_waves.h"

int main(int argc, char **argv) {
    const int steps = argc > 1 ? atoi(argv[1]) : 150, n = argc > 2 ? atoi(argv[2]) : 256, cascades = 3;
    const double dt = 1.0 / 50.0;   /* water.gd:51 */

    ow_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.map_size = n; cfg.num_cascades = cascades; cfg.device_id = -1; cfg.depth = 20.0f;
    ow_context *ctx = NULL;
    ow_spray *spray = NULL;
    if (ow_create(&cfg, &ctx) != OW_OK) { fprintf(stderr, "ow_create: %s\n", ow_last_error()); return 1; }

    static const float tile[3] = {88.0f, 57.0f, 16.0f}, wind[3] = {10.0f, 5.0f, 20.0f}, dir[3] = {20.0f, 15.0f, 20.0f};
    static const float fetch[3] = {150.0f, 150.0f, 550.0f}, spread[3] = {0.2f, 0.4f, 0.4f}, whitecap[3] = {0.5f, 0.5f, 0.25f}, foam[3] = {8.0f, 0.0f, 3.0f};
    ow_cascade_params par[3];
    float map_scales[3][4];
    for (int i = 0; i < cascades; ++i) {
        ow_cascade_params_default(&par[i]);
        par[i].tile_length[0] = par[i].tile_length[1] = tile[i];
        par[i].wind_speed = wind[i]; par[i].wind_direction = dir[i]; par[i].fetch_length = fetch[i];
        par[i].spread = spread[i]; par[i].whitecap = whitecap[i]; par[i].foam_amount = foam[i];
        par[i].spectrum_seed[0] = 1000 + 17 * i; par[i].spectrum_seed[1] = -2000 + 31 * i;
        par[i].time = 120.0 + 3.14159265358979323846 * i;
        map_scales[i][0] = map_scales[i][1] = 1.0f / tile[i];
        map_scales[i][2] = (float)par[i].displacement_scale;
        map_scales[i][3] = (float)par[i].normal_scale;
    }

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
        ow_spray_instance *inst = (ow_spray_instance *)malloc((size_t)opts.amount * sizeof(ow_spray_instance));
        uint32_t *draw = (uint32_t *)malloc((size_t)opts.amount * sizeof(uint32_t));
        uint32_t live = 0;
        double time = 0.0;
        uint64_t taken = 0, restarts = 0, spawned = 0, rejected = 0;
        int finite = 1, ascending = 1;
        if (!inst || !draw) { fprintf(stderr, "out of memory\n"); return 1; }
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
        free(inst); free(draw);
    }
    ow_spray_destroy(ctx, spray);
    ow_destroy(ctx);
    return 0;
fail:
    fprintf(stderr, "ocean_waves: %s\n", ow_last_error());
    ow_spray_destroy(ctx, spray);
    ow_destroy(ctx);
    return 1;
}

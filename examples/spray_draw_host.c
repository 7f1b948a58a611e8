/* spray_draw_host.c -- the reference scene with its sea spray, from plain C99: creates a context over the three cascades and the
 * WaterSprayEmitter of main.tscn:133-140, ticks the waves and steps the emitter behind them, then draws a grid mesh with
 * ow_mesh_draw_async and the emitter's billboards over it with ow_billboard_draw_async -- both into device buffers, in the context's stream
 * order, with no synchronisation in between -- copies the picture back and writes a binary PPM.
 *   gcc -O2 -std=c99 -Iinclude examples/spray_draw_host.c -o spray_draw_host -Lgodotoceanwaves_amd -locean_waves -L/opt/rocm/lib -lamdhip64 \
 *       -Wl,-rpath,$PWD/godotoceanwaves_amd -Wl,-rpath,/opt/rocm/lib -lm && ./spray_draw_host [out.ppm [width height [steps [map_size [amount]]]]]
 * The scene is mesh_host.c's and spray_host.c's.  The two textures are scene.h's procedural ones -- a round puff with a soft edge for the
 * albedo, a tiling value noise for the dissolve.  Prints key=value pairs: the image size, the live particles, the billboards drawn and
 * culled, the pixels that received spray and whether every colour is finite. */
#include "scene.h"

int main(int argc, char **argv) {
    const char *path = argc > 1 ? argv[1] : "spray.ppm";
    const int width = argc > 3 ? atoi(argv[2]) : 320, height = argc > 3 ? atoi(argv[3]) : 200;
    const int steps = scene_arg(argc, argv, 4, 150), n = scene_arg(argc, argv, 5, 256), cascades = SCENE_CASCADES;
    const double dt = 1.0 / 50.0;   /* water.gd:51 */
    int status = 1;

    ow_config cfg;
    scene_config(&cfg, n);
    ow_context *ctx = NULL;
    ow_mesh *mesh = NULL;
    ow_spray *spray = NULL;
    ow_billboard_material *material = NULL;
    unsigned char *rgba = NULL;
    ow_render_pixel *px = NULL;
    void *rgba_dev = NULL, *px_dev = NULL;
    if (ow_create(&cfg, &ctx) != OW_OK) { fprintf(stderr, "ow_create: %s\n", ow_last_error()); return 1; }

    ow_cascade_params par[SCENE_CASCADES];
    float map_scales[SCENE_CASCADES][4];
    scene_cascades(par, map_scales);
    if (scene_bad_size(width, height, 1)) goto out;

    ow_spray_options so;
    ow_spray_options_default(&so);   /* mat_spray.tres, main.tscn:133-140 */
    if (argc > 6) so.amount = (uint32_t)atoi(argv[6]);
    if (ow_spray_create(ctx, &so, &spray) != OW_OK) goto fail;

    {   /* the material: sea_spray.gdshader's uniforms as the scene sets them, over the two procedural textures */
        static unsigned char albedo[SCENE_TEX * SCENE_TEX * 4], dissolve[SCENE_TEX * SCENE_TEX * 4];
        ow_billboard_material_options mo;
        scene_textures(albedo, dissolve);
        ow_billboard_material_options_default(&mo);
        if (ow_billboard_material_create(ctx, &mo, albedo, SCENE_TEX, SCENE_TEX, dissolve, SCENE_TEX, SCENE_TEX, &material) != OW_OK) goto fail;
    }
    if (scene_grid_create(ctx, SCENE_CELLS, SCENE_CELL, &mesh)) goto out;

    ow_camera cam;
    float origin[3];
    scene_camera(&cam, width, height);
    scene_clipmap_origin(&cam, SCENE_CELL, origin);
    ow_mesh_options opts;
    scene_mesh_options(&opts, &cam);

    const size_t count = (size_t)width * (size_t)height;
    if (hipMalloc(&rgba_dev, count * 4) || hipMalloc(&px_dev, count * sizeof(ow_render_pixel))) { fprintf(stderr, "hipMalloc failed\n"); goto out; }

    for (int k = 0; k < steps; ++k) {
        if (ow_update_all(ctx, dt, par, cascades) != OW_OK) goto fail;
        if (ow_spray_step(ctx, spray, dt, &map_scales[0][0], cascades) != OW_OK) goto fail;   /* enqueued behind the tick */
    }
    /* the frame: the water, then the spray over it, both behind the last step; nothing is synchronised until the copies below */
    if (ow_mesh_draw_async(ctx, mesh, &cam, origin, &map_scales[0][0], cascades, &opts, rgba_dev, (ow_render_pixel *)px_dev) != OW_OK) goto fail;
    if (ow_billboard_draw_async(ctx, spray, material, &cam, NULL, (ow_render_pixel *)px_dev, rgba_dev) != OW_OK) goto fail;
    if (ow_sync(ctx) != OW_OK) goto fail;

    rgba = (unsigned char *)malloc(count * 4);
    px = (ow_render_pixel *)malloc(count * sizeof(ow_render_pixel));
    if (!rgba || !px) { fprintf(stderr, "out of memory\n"); goto out; }
    if (hipMemcpy(rgba, rgba_dev, count * 4, HIP_DEVICE_TO_HOST) || hipMemcpy(px, px_dev, count * sizeof(ow_render_pixel), HIP_DEVICE_TO_HOST)) {
        fprintf(stderr, "hipMemcpy failed\n");
        goto out;
    }
    uint64_t culled = 0, drawn = 0;
    uint32_t live = 0;
    if (ow_billboard_draw_stats(ctx, NULL, &culled, &drawn, NULL) != OW_OK) goto fail;
    if (ow_spray_read(ctx, spray, NULL, NULL, NULL, &live) != OW_OK) goto fail;
    if (scene_write_ppm(path, rgba, width, height)) goto out;

    {
        size_t sprayed = 0, fragments = 0;
        int finite = 1;
        for (size_t i = 0; i < count; ++i) {
            for (int k = 0; k < 3; ++k) finite &= isfinite(px[i].color[k]) != 0;
            sprayed += px[i].reserved[1] > 0;
            fragments += px[i].reserved[1];
        }
        printf("file=%s width=%d height=%d steps=%d amount=%u live=%u drawn=%llu culled=%llu sprayed_pixels=%llu fragments=%llu finite=%d\n", path, width,
               height, steps, (unsigned)so.amount, (unsigned)live, (unsigned long long)drawn, (unsigned long long)culled, (unsigned long long)sprayed,
               (unsigned long long)fragments, finite);
    }
    status = 0;
    goto out;
fail:
    fprintf(stderr, "ocean_waves: %s\n", ow_last_error());
out:
    free(rgba); free(px);
    (void)hipFree(rgba_dev); (void)hipFree(px_dev);
    ow_billboard_material_destroy(ctx, material);
    ow_spray_destroy(ctx, spray);
    ow_mesh_destroy(ctx, mesh);
    ow_destroy(ctx);
    return status;
}

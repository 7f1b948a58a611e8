/* mist_host.c -- the sea, 36 crates and THE SHAFTS THEIR SHADOWS CUT INTO THE SEA MIST, from plain C99: the reference scene's three
 * cascades, scene.h's crates floating on them, a shadow map of the crates from the scene's low sun, and the frame drawn in the
 * order water, solids, shadows, environment, mist, present -- ow_mesh_draw_async, ow_solid_draw_async, ow_shadow_map_begin / _cast,
 * ow_shadow_apply_async, ow_environment_apply_async, ow_mist_apply_async (the map's casters shadow the mist), ow_present_async -- in the
 * context's stream order with no synchronisation in between; the sRGB picture is copied back and written as a binary PPM.
 *   gcc -O2 -std=c99 -Iinclude examples/mist_host.c -o mist_host -Lgodotoceanwaves_amd -locean_waves -L/opt/rocm/lib -lamdhip64 \
 *       -Wl,-rpath,$PWD/godotoceanwaves_amd -Wl,-rpath,/opt/rocm/lib -lm && ./mist_host [out.ppm [width height [steps [map_size [downsample [shadow_size [slices]]]]]]]
 * width x height is the size of the PPM; the records are drawn at downsample (1 .. 4, default 2) times that.  Prints key=value pairs: the
 * image size, the record size, the shadow map's size, the mist pass's counters, the pixels it marked and whether every resolved linear
 * colour is finite. */
#include "scene.h"

#define SUBSTEPS 4
#define SHADOW_SIZE 1024

static ow_rigid_body bodies[SCENE_CRATES];
static ow_hull_point hull[SCENE_CRATES * SCENE_PER_CRATE];

int main(int argc, char **argv) {
    const char *path = argc > 1 ? argv[1] : "mist.ppm";
    const int out_width = argc > 3 ? atoi(argv[2]) : 320, out_height = argc > 3 ? atoi(argv[3]) : 200, down = scene_arg(argc, argv, 6, 2);
    const int steps = scene_arg(argc, argv, 4, 150), n = scene_arg(argc, argv, 5, 256), cascades = SCENE_CASCADES;
    const double dt = 1.0 / 50.0;   /* water.gd:51 */
    const int shadow_size = scene_arg(argc, argv, 7, SHADOW_SIZE), slices = scene_arg(argc, argv, 8, 0);
    int status = 1;

    ow_config cfg;
    scene_config(&cfg, n);
    ow_context *ctx = NULL;
    ow_mesh *mesh = NULL;
    ow_bodies *set = NULL;
    ow_solid *solid = NULL;
    ow_shadow_map *shadow = NULL;
    unsigned char *rgba = NULL;
    float *linear = NULL;
    ow_render_pixel *px = NULL;
    void *rgba_dev = NULL, *px_dev = NULL, *linear_dev = NULL;
    if (ow_create(&cfg, &ctx) != OW_OK) { fprintf(stderr, "ow_create: %s\n", ow_last_error()); return 1; }

    ow_cascade_params par[SCENE_CASCADES];
    float map_scales[SCENE_CASCADES][4];
    scene_cascades(par, map_scales);
    if (scene_bad_size(out_width, out_height, down)) goto out;
    const int width = out_width * down, height = out_height * down;   /* the records */

    if (ow_shadow_map_create(ctx, shadow_size, &shadow) != OW_OK) goto fail;

    {   /* the crates: their states and voxelised hulls, and the same box as a shape */
        float corners[SCENE_BOX_VERTICES][3];
        int32_t idx[SCENE_BOX_TRIANGLES][3];
        scene_crates(bodies, hull);
        if (ow_bodies_create(ctx, bodies, SCENE_CRATES, hull, SCENE_CRATES * SCENE_PER_CRATE, &set) != OW_OK) goto fail;
        scene_box(corners, idx);
        if (ow_solid_create(ctx, &corners[0][0], SCENE_BOX_VERTICES, &idx[0][0], SCENE_BOX_TRIANGLES, &solid) != OW_OK) goto fail;
    }
    if (scene_grid_create(ctx, SCENE_CELLS, SCENE_CELL, &mesh)) goto out;

    ow_camera cam;
    float origin[3];
    scene_camera(&cam, width, height);
    scene_clipmap_origin(&cam, SCENE_CELL, origin);
    ow_mesh_options opts;
    scene_mesh_options(&opts, &cam);

    const size_t count = (size_t)width * (size_t)height, out_count = (size_t)out_width * (size_t)out_height;
    if (hipMalloc(&rgba_dev, out_count * 4) || hipMalloc(&linear_dev, out_count * 16) || hipMalloc(&px_dev, count * sizeof(ow_render_pixel))) { fprintf(stderr, "hipMalloc failed\n"); goto out; }

    ow_bodies_options bo;
    memset(&bo, 0, sizeof bo);
    bo.buoyancy.flags = OW_BUOYANCY_WARM_START;
    for (int k = 0; k < steps; ++k) {
        if (ow_update_all(ctx, dt, par, cascades) != OW_OK) goto fail;
        if (ow_bodies_step(ctx, set, &map_scales[0][0], cascades, &bo, SUBSTEPS, dt / SUBSTEPS) != OW_OK) goto fail;
    }
    /* the frame: water, crates, shadows, sky colour and fog, mist with the crates' shafts, present, all behind the last step */
    ow_shadow_frame frame;
    ow_shadow_frame_default(&frame);   /* the scene's sun, main.tscn:113 */
    frame.center[2] = 10.0f;           /* the middle of the crates; 80 m a side holds them and their 13 m shadows */
    frame.half_extent = 40.0f;
    frame.depth_range = 80.0f;
    ow_shadow_options sho;
    ow_shadow_options_default(&sho);   /* main.tscn:114-116 */
    sho.flags = OW_SHADOW_RECEIVE_WATER;
    ow_mist_options mo;
    ow_mist_options_init(&mo);         /* main.tscn:35-37, :100-104, :142-144 */
    mo.slices = slices;
    ow_present_options po;
    ow_present_options_default(&po);   /* main.tscn:25, :38-41 */
    po.downsample = down;
    if (ow_mesh_draw_async(ctx, mesh, &cam, origin, &map_scales[0][0], cascades, &opts, NULL, (ow_render_pixel *)px_dev) != OW_OK) goto fail;
    if (ow_solid_draw_async(ctx, solid, set, 0, SCENE_CRATES, &cam, NULL, (ow_render_pixel *)px_dev, NULL) != OW_OK) goto fail;
    if (ow_shadow_map_begin(ctx, shadow, &frame) != OW_OK) goto fail;
    if (ow_shadow_map_cast(ctx, shadow, solid, set, 0, SCENE_CRATES) != OW_OK) goto fail;   /* the poses stay on the device */
    if (ow_shadow_apply_async(ctx, shadow, &cam, &sho, (ow_render_pixel *)px_dev, NULL) != OW_OK) goto fail;
    if (ow_environment_apply_async(ctx, NULL, &cam, NULL, (ow_render_pixel *)px_dev) != OW_OK) goto fail;   /* main.tscn:22-34 */
    if (ow_mist_apply_async(ctx, shadow, &cam, &mo, (ow_render_pixel *)px_dev, NULL) != OW_OK) goto fail;
    if (ow_present_async(ctx, &cam, &po, (const ow_render_pixel *)px_dev, rgba_dev, (float *)linear_dev) != OW_OK) goto fail;
    if (ow_sync(ctx) != OW_OK) goto fail;

    rgba = (unsigned char *)malloc(out_count * 4);
    linear = (float *)malloc(out_count * 16);
    px = (ow_render_pixel *)malloc(count * sizeof(ow_render_pixel));
    if (!rgba || !px || !linear) { fprintf(stderr, "out of memory\n"); goto out; }
    if (hipMemcpy(rgba, rgba_dev, out_count * 4, HIP_DEVICE_TO_HOST) || hipMemcpy(linear, linear_dev, out_count * 16, HIP_DEVICE_TO_HOST) ||
        hipMemcpy(px, px_dev, count * sizeof(ow_render_pixel), HIP_DEVICE_TO_HOST)) {
        fprintf(stderr, "hipMemcpy failed\n");
        goto out;
    }
    if (scene_write_ppm(path, rgba, out_width, out_height)) goto out;

    {
        size_t misted = 0, crate_pixels = 0;
        uint64_t passes = 0, pixels = 0, fetched = 0, shadowed = 0;
        if (ow_mist_stats(ctx, &passes, &pixels, &fetched, &shadowed) != OW_OK) goto fail;
        int finite = 1;
        for (size_t i = 0; i < count; ++i) {
            misted += (px[i].status & OW_RAY_MIST) != 0;
            crate_pixels += (px[i].status & OW_RAY_SOLID) != 0;
        }
        for (size_t i = 0; i < 4 * out_count; ++i) finite &= isfinite(linear[i]) != 0;
        printf("file=%s width=%d height=%d downsample=%d record_width=%d record_height=%d steps=%d crates=%d shadow_size=%d passes=%llu pixels=%llu "
               "slices_fetched=%llu slices_shadowed=%llu misted_pixels=%llu crate_pixels=%llu finite=%d\n",
               path, out_width, out_height, down, width, height, steps, SCENE_CRATES, shadow_size, (unsigned long long)passes, (unsigned long long)pixels,
               (unsigned long long)fetched, (unsigned long long)shadowed, (unsigned long long)misted, (unsigned long long)crate_pixels, finite);
    }
    status = 0;
    goto out;
fail:
    fprintf(stderr, "ocean_waves: %s\n", ow_last_error());
out:
    free(rgba); free(px); free(linear);
    (void)hipFree(rgba_dev); (void)hipFree(px_dev); (void)hipFree(linear_dev);
    ow_shadow_map_destroy(ctx, shadow);
    ow_solid_destroy(ctx, solid);
    ow_bodies_destroy(ctx, set);
    ow_mesh_destroy(ctx, mesh);
    ow_destroy(ctx);
    return status;
}

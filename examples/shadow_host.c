/* shadow_host.c -- sky_light_host.c's frame of the sea WITH THE CRATES' SUN SHADOWS, from plain C99: the same scene (the reference scene's
 * three cascades, 36 crates floating on them, the WaterSprayEmitter, a small procedural gradient panorama and its radiance pyramid), with a
 * shadow map of the crates from the scene's sun (ow_shadow_map_create once; ow_shadow_map_begin and ow_shadow_map_cast from the body set's
 * resident poses every frame) and the frame drawn in the order water, solids, shadows, sky light, environment, billboards, present --
 * ow_mesh_draw_async, ow_solid_draw_async, ow_shadow_apply_async with OW_SHADOW_RECEIVE_WATER (the crates darken the water beside them
 * and each other), ow_radiance_light_apply_async, ow_environment_apply_async, ow_billboard_draw_async, ow_present_async -- in the context's
 * stream order with no synchronisation in between; the sRGB picture is copied back and written as a binary PPM.
 *   gcc -O2 -std=c99 -Iinclude examples/shadow_host.c -o shadow_host -Lgodotoceanwaves_amd -locean_waves -L/opt/rocm/lib -lamdhip64 \
 *       -Wl,-rpath,$PWD/godotoceanwaves_amd -Wl,-rpath,/opt/rocm/lib -lm && ./shadow_host [out.ppm [width height [steps [map_size [amount [downsample [shadow_size]]]]]]]
 * width x height is the size of the PPM; the records are drawn at downsample (1 .. 4, default 2) times that.  Prints key=value pairs: the
 * image size, the record size, the shadow map's size and counters, the pixels the shadow pass took as receivers, those of them that are
 * water and those that are crates with their sun dimmed, the pixels that show a crate, the pixels that received spray and whether every
 * resolved linear colour is finite. */
#include "scene.h"

#define SUBSTEPS 4
#define SHADOW_SIZE 1024

static ow_rigid_body bodies[SCENE_CRATES];
static ow_hull_point hull[SCENE_CRATES * SCENE_PER_CRATE];

int main(int argc, char **argv) {
    const char *path = argc > 1 ? argv[1] : "shadow.ppm";
    const int out_width = argc > 3 ? atoi(argv[2]) : 320, out_height = argc > 3 ? atoi(argv[3]) : 200, down = scene_arg(argc, argv, 7, 2);
    const int steps = scene_arg(argc, argv, 4, 150), n = scene_arg(argc, argv, 5, 256), cascades = SCENE_CASCADES;
    const double dt = 1.0 / 50.0;   /* water.gd:51 */
    const int shadow_size = scene_arg(argc, argv, 8, SHADOW_SIZE);
    int status = 1;

    ow_config cfg;
    scene_config(&cfg, n);
    ow_context *ctx = NULL;
    ow_mesh *mesh = NULL;
    ow_spray *spray = NULL;
    ow_billboard_material *material = NULL;
    ow_bodies *set = NULL;
    ow_solid *solid = NULL;
    ow_sky *sky = NULL;
    ow_radiance *radiance = NULL;
    ow_shadow_map *shadow = NULL;
    int32_t levels = 0;
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

    {   /* the sky: stands in for main.tscn's PanoramaSkyMaterial */
        static unsigned char panorama[SCENE_PANO_W * SCENE_PANO_H * 4];
        scene_panorama(panorama);
        if (ow_sky_create(ctx, NULL, panorama, SCENE_PANO_W, SCENE_PANO_H, &sky) != OW_OK) goto fail;
        /* its radiance pyramid: six levels from 256 x 128 down to 8 x 4, 64 samples a texel, and the 32 x 16 irradiance */
        if (ow_radiance_create(ctx, sky, NULL, &radiance) != OW_OK) goto fail;
        if (ow_radiance_level(ctx, radiance, 0, &levels, NULL, NULL, NULL) != OW_OK) goto fail;
    }

    if (ow_shadow_map_create(ctx, shadow_size, &shadow) != OW_OK) goto fail;

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
    opts.ambient_color[0] = opts.ambient_color[1] = opts.ambient_color[2] = 0.0f;   /* the sky lights the frame: no flat ambient */
    ow_solid_options sopts;
    ow_solid_options_default(&sopts);
    sopts.ambient_color[0] = sopts.ambient_color[1] = sopts.ambient_color[2] = 0.0f;

    const size_t count = (size_t)width * (size_t)height, out_count = (size_t)out_width * (size_t)out_height;
    if (hipMalloc(&rgba_dev, out_count * 4) || hipMalloc(&linear_dev, out_count * 16) || hipMalloc(&px_dev, count * sizeof(ow_render_pixel))) { fprintf(stderr, "hipMalloc failed\n"); goto out; }

    ow_bodies_options bo;
    memset(&bo, 0, sizeof bo);
    bo.buoyancy.flags = OW_BUOYANCY_WARM_START;
    for (int k = 0; k < steps; ++k) {
        if (ow_update_all(ctx, dt, par, cascades) != OW_OK) goto fail;
        if (ow_bodies_step(ctx, set, &map_scales[0][0], cascades, &bo, SUBSTEPS, dt / SUBSTEPS) != OW_OK) goto fail;
        if (ow_spray_step(ctx, spray, dt, &map_scales[0][0], cascades) != OW_OK) goto fail;   /* enqueued behind the tick */
    }
    /* the frame: water, crates, shadows, sky light, sky and fog, spray, present, all behind the last step; nothing is synchronised until the copies below */
    ow_shadow_frame frame;
    ow_shadow_frame_default(&frame);   /* the scene's sun, main.tscn:113 */
    frame.center[2] = 10.0f;           /* the middle of the crates; 80 m a side holds them and their 13 m shadows */
    frame.half_extent = 40.0f;
    frame.depth_range = 80.0f;
    ow_shadow_options sho;
    ow_shadow_options_default(&sho);   /* main.tscn:114-116 */
    sho.flags = OW_SHADOW_RECEIVE_WATER;
    ow_present_options po;
    ow_present_options_default(&po);   /* main.tscn:25, :38-41 */
    po.downsample = down;
    if (ow_mesh_draw_async(ctx, mesh, &cam, origin, &map_scales[0][0], cascades, &opts, NULL, (ow_render_pixel *)px_dev) != OW_OK) goto fail;
    if (ow_solid_draw_async(ctx, solid, set, 0, SCENE_CRATES, &cam, &sopts, (ow_render_pixel *)px_dev, NULL) != OW_OK) goto fail;
    if (ow_shadow_map_begin(ctx, shadow, &frame) != OW_OK) goto fail;
    if (ow_shadow_map_cast(ctx, shadow, solid, set, 0, SCENE_CRATES) != OW_OK) goto fail;   /* the poses stay on the device */
    if (ow_shadow_apply_async(ctx, shadow, &cam, &sho, (ow_render_pixel *)px_dev, NULL) != OW_OK) goto fail;
    if (ow_radiance_light_apply_async(ctx, radiance, &cam, NULL, (ow_render_pixel *)px_dev) != OW_OK) goto fail;   /* main.tscn:16-24 */
    if (ow_environment_apply_async(ctx, sky, &cam, NULL, (ow_render_pixel *)px_dev) != OW_OK) goto fail;   /* main.tscn:22-34 */
    if (ow_billboard_draw_async(ctx, spray, material, &cam, NULL, (ow_render_pixel *)px_dev, NULL) != OW_OK) goto fail;
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
        size_t sprayed = 0, crate_pixels = 0, receivers = 0, water_receivers = 0, lit = 0;
        uint64_t casts = 0, skipped = 0, culled = 0, drawn = 0;
        if (ow_shadow_stats(ctx, shadow, &casts, &skipped, &culled, &drawn, NULL) != OW_OK) goto fail;
        int finite = 1;
        for (size_t i = 0; i < count; ++i) {
            lit += (px[i].status & OW_RAY_SKY_LIT) != 0;
            receivers += (px[i].status & OW_RAY_SHADOWED) != 0;
            water_receivers += (px[i].status & OW_RAY_SHADOWED) != 0 && (px[i].status & OW_RAY_SOLID) == 0;
            crate_pixels += (px[i].status & OW_RAY_SOLID) != 0;
            sprayed += px[i].reserved[1] > 0;
        }
        for (size_t i = 0; i < 4 * out_count; ++i) finite &= isfinite(linear[i]) != 0;
        printf("file=%s width=%d height=%d downsample=%d record_width=%d record_height=%d steps=%d crates=%d shadow_size=%d casts=%llu skipped_instances=%llu "
               "triangles_culled=%llu triangles_cast=%llu receivers=%llu water_receivers=%llu lit_pixels=%llu crate_pixels=%llu sprayed_pixels=%llu finite=%d\n",
               path, out_width, out_height, down, width, height, steps, SCENE_CRATES, shadow_size, (unsigned long long)casts, (unsigned long long)skipped,
               (unsigned long long)culled, (unsigned long long)drawn, (unsigned long long)receivers, (unsigned long long)water_receivers,
               (unsigned long long)lit, (unsigned long long)crate_pixels, (unsigned long long)sprayed, finite);
    }
    status = 0;
    goto out;
fail:
    fprintf(stderr, "ocean_waves: %s\n", ow_last_error());
out:
    free(rgba); free(px); free(linear);
    (void)hipFree(rgba_dev); (void)hipFree(px_dev); (void)hipFree(linear_dev);
    ow_shadow_map_destroy(ctx, shadow);
    ow_radiance_destroy(ctx, radiance);
    ow_sky_destroy(ctx, sky);
    ow_solid_destroy(ctx, solid);
    ow_bodies_destroy(ctx, set);
    ow_billboard_material_destroy(ctx, material);
    ow_spray_destroy(ctx, spray);
    ow_mesh_destroy(ctx, mesh);
    ow_destroy(ctx);
    return status;
}

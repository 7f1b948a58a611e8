/* mirror_host.c -- the sea with crates AND THEIR REFLECTIONS IN THE WATER, from plain C99: sky_light_host.c's scene (the reference scene's
 * three cascades, crates floating on them, a small procedural gradient panorama and its radiance pyramid) seen from low over the water, the
 * frame drawn in the order water, solids, mirror, environment, present -- ow_mesh_draw_async and ow_solid_draw_async with their flat
 * ambient_color set to 0, ow_mirror_apply_async (everything ow_radiance_light_apply does, and the crates' lit colour where a water pixel's
 * mirror ray meets one), ow_environment_apply_async, ow_present_async -- in the context's stream order with no synchronisation in between;
 * the sRGB picture is copied back and written as a binary PPM.  The same records go through ow_radiance_light_apply_async as well, for
 * comparison: only water pixels may differ.  The scene's pieces (cascades, crates, grid, panorama) are scene.h's.
 *   gcc -O2 -std=c99 -Iinclude examples/mirror_host.c -o mirror_host -Lgodotoceanwaves_amd -locean_waves -L/opt/rocm/lib -lamdhip64 \
 *       -Wl,-rpath,$PWD/godotoceanwaves_amd -Wl,-rpath,/opt/rocm/lib -lm && ./mirror_host [out.ppm [width height [steps [map_size [sky_only.ppm [kinds.bin]]]]]]
 * sky_only.ppm: the comparison frame; kinds.bin: one byte a pixel, 0 sky, 1 water, 2 crate.  Prints key=value pairs: the image size, the
 * pixels that show a crate, the pixels that reflect one, the pass's counters, the pixels in which the two frames differ (water, and everything
 * else: 0) and whether every resolved linear colour is finite. */
#include "scene.h"

#define SUBSTEPS 4

static ow_rigid_body bodies[SCENE_CRATES];
static ow_hull_point hull[SCENE_CRATES * SCENE_PER_CRATE];

int main(int argc, char **argv) {
    const char *path = argc > 1 ? argv[1] : "mirror.ppm", *ref_path = argc > 6 ? argv[6] : NULL, *kinds_path = argc > 7 ? argv[7] : NULL;
    const int width = argc > 3 ? atoi(argv[2]) : 320, height = argc > 3 ? atoi(argv[3]) : 200;
    const int steps = scene_arg(argc, argv, 4, 150), n = scene_arg(argc, argv, 5, 256), cascades = SCENE_CASCADES;
    const double dt = 1.0 / 50.0;   /* water.gd:51 */
    int status = 1;

    ow_config cfg;
    scene_config(&cfg, n);
    ow_context *ctx = NULL;
    ow_mesh *mesh = NULL;
    ow_bodies *set = NULL;
    ow_solid *solid = NULL;
    ow_sky *sky = NULL;
    ow_radiance *radiance = NULL;
    unsigned char *rgba = NULL, *ref = NULL, *kinds = NULL;
    float *linear = NULL;
    ow_render_pixel *px = NULL;
    void *rgba_dev = NULL, *px_dev = NULL, *ref_dev = NULL, *linear_dev = NULL;
    if (ow_create(&cfg, &ctx) != OW_OK) { fprintf(stderr, "ow_create: %s\n", ow_last_error()); return 1; }

    ow_cascade_params par[SCENE_CASCADES];
    float map_scales[SCENE_CASCADES][4];
    scene_cascades(par, map_scales);
    if (scene_bad_size(width, height, 1)) goto out;

    {   /* the sky and its radiance pyramid: six levels from 256 x 128 down to 8 x 4, 64 samples a texel, and the 32 x 16 irradiance */
        static unsigned char panorama[SCENE_PANO_W * SCENE_PANO_H * 4];
        scene_panorama(panorama);
        if (ow_sky_create(ctx, NULL, panorama, SCENE_PANO_W, SCENE_PANO_H, &sky) != OW_OK) goto fail;
        if (ow_radiance_create(ctx, sky, NULL, &radiance) != OW_OK) goto fail;
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
    scene_camera(&cam, width, height);
    {   /* its own pose: 3.5 m over the water, 12 m in front of the first row of crates, looking along +z and 8 degrees down: the crates stand over their images */
        static const float basis[9] = {-1.0f, 0.0f, 0.0f, 0.0f, 0.990268f, 0.139173f, 0.0f, 0.139173f, -0.990268f};
        memcpy(cam.basis, basis, sizeof basis);
        cam.position[0] = 0.0f; cam.position[1] = 3.5f; cam.position[2] = -17.0f;
        cam.fov_y_degrees = 60.0f;
    }
    float origin[3];
    scene_clipmap_origin(&cam, SCENE_CELL, origin);

    ow_mesh_options opts;
    scene_mesh_options(&opts, &cam);
    opts.ambient_color[0] = opts.ambient_color[1] = opts.ambient_color[2] = 0.0f;   /* the sky lights the frame: no flat ambient */
    ow_solid_options sopts;
    ow_solid_options_default(&sopts);
    sopts.ambient_color[0] = sopts.ambient_color[1] = sopts.ambient_color[2] = 0.0f;
    ow_mirror_options mo;
    ow_mirror_options_init(&mo);                    /* the draw's colour and sun; its ambient as the draw has it: 0 */
    mo.ambient_color[0] = mo.ambient_color[1] = mo.ambient_color[2] = 0.0f;

    const size_t count = (size_t)width * (size_t)height;
    if (hipMalloc(&rgba_dev, count * 4) || hipMalloc(&linear_dev, count * 16) || hipMalloc(&px_dev, count * sizeof(ow_render_pixel)) ||
        hipMalloc(&ref_dev, count * sizeof(ow_render_pixel))) { fprintf(stderr, "hipMalloc failed\n"); goto out; }
    rgba = (unsigned char *)malloc(count * 4);
    ref = (unsigned char *)malloc(count * 4);
    kinds = (unsigned char *)malloc(count);
    linear = (float *)malloc(count * 16);
    px = (ow_render_pixel *)malloc(count * sizeof(ow_render_pixel));
    if (!rgba || !ref || !kinds || !px || !linear) { fprintf(stderr, "out of memory\n"); goto out; }

    ow_bodies_options bo;
    memset(&bo, 0, sizeof bo);
    bo.buoyancy.flags = OW_BUOYANCY_WARM_START;
    for (int k = 0; k < steps; ++k) {
        if (ow_update_all(ctx, dt, par, cascades) != OW_OK) goto fail;
        if (ow_bodies_step(ctx, set, &map_scales[0][0], cascades, &bo, SUBSTEPS, dt / SUBSTEPS) != OW_OK) goto fail;
    }
    /* the frame: water and crates, then the same records twice -- through the sky pass alone, and through the mirror pass */
    ow_present_options po;
    ow_present_options_default(&po);   /* main.tscn:25, :38-41 */
    po.downsample = 1;
    if (ow_mesh_draw_async(ctx, mesh, &cam, origin, &map_scales[0][0], cascades, &opts, NULL, (ow_render_pixel *)px_dev) != OW_OK) goto fail;
    if (ow_solid_draw_async(ctx, solid, set, 0, SCENE_CRATES, &cam, &sopts, (ow_render_pixel *)px_dev, NULL) != OW_OK) goto fail;
    if (ow_sync(ctx) != OW_OK) goto fail;
    if (hipMemcpy(ref_dev, px_dev, count * sizeof(ow_render_pixel), HIP_DEVICE_TO_DEVICE)) { fprintf(stderr, "hipMemcpy failed\n"); goto out; }
    if (ow_radiance_light_apply_async(ctx, radiance, &cam, NULL, (ow_render_pixel *)ref_dev) != OW_OK) goto fail;   /* main.tscn:16-24 */
    if (ow_environment_apply_async(ctx, sky, &cam, NULL, (ow_render_pixel *)ref_dev) != OW_OK) goto fail;
    if (ow_present_async(ctx, &cam, &po, (const ow_render_pixel *)ref_dev, rgba_dev, NULL) != OW_OK) goto fail;
    if (ow_sync(ctx) != OW_OK) goto fail;
    if (hipMemcpy(ref, rgba_dev, count * 4, HIP_DEVICE_TO_HOST)) { fprintf(stderr, "hipMemcpy failed\n"); goto out; }
    if (ow_mirror_apply_async(ctx, radiance, solid, set, 0, SCENE_CRATES, &cam, &mo, (ow_render_pixel *)px_dev, NULL) != OW_OK) goto fail;
    if (ow_environment_apply_async(ctx, sky, &cam, NULL, (ow_render_pixel *)px_dev) != OW_OK) goto fail;   /* main.tscn:22-34 */
    if (ow_present_async(ctx, &cam, &po, (const ow_render_pixel *)px_dev, rgba_dev, (float *)linear_dev) != OW_OK) goto fail;
    if (ow_sync(ctx) != OW_OK) goto fail;
    if (hipMemcpy(rgba, rgba_dev, count * 4, HIP_DEVICE_TO_HOST) || hipMemcpy(linear, linear_dev, count * 16, HIP_DEVICE_TO_HOST) ||
        hipMemcpy(px, px_dev, count * sizeof(ow_render_pixel), HIP_DEVICE_TO_HOST)) {
        fprintf(stderr, "hipMemcpy failed\n");
        goto out;
    }
    if (scene_write_ppm(path, rgba, width, height)) goto out;
    if (ref_path && scene_write_ppm(ref_path, ref, width, height)) goto out;

    {
        size_t crate_pixels = 0, water_pixels = 0, mirror_pixels = 0, differ_water = 0, differ_other = 0;
        uint64_t passes = 0, pixels = 0, rays = 0, passed = 0, pairs = 0, hits = 0;
        int finite = 1;
        for (size_t i = 0; i < count; ++i) {
            const int hit = (px[i].status & OW_RAY_HIT) != 0, crate = (px[i].status & OW_RAY_SOLID) != 0;
            kinds[i] = (unsigned char)(crate ? 2 : hit ? 1 : 0);
            crate_pixels += crate;
            water_pixels += hit && !crate;
            mirror_pixels += (px[i].status & OW_RAY_MIRROR) != 0;
            if (memcmp(rgba + 4 * i, ref + 4 * i, 4) != 0) {
                if (kinds[i] == 1) ++differ_water;
                else ++differ_other;
            }
        }
        for (size_t i = 0; i < 4 * count; ++i) finite &= isfinite(linear[i]) != 0;
        if (kinds_path && scene_write_file(kinds_path, kinds, count)) goto out;
        if (ow_mirror_stats(ctx, &passes, &pixels, &rays, &passed, &pairs, &hits) != OW_OK) goto fail;
        printf("file=%s width=%d height=%d steps=%d crates=%d water_pixels=%llu crate_pixels=%llu mirror_pixels=%llu passes=%llu pixels=%llu rays_cast=%llu "
               "sphere_tests_passed=%llu pairs_tested=%llu rays_hit=%llu differing_water_pixels=%llu differing_other_pixels=%llu finite=%d\n",
               path, width, height, steps, SCENE_CRATES, (unsigned long long)water_pixels, (unsigned long long)crate_pixels, (unsigned long long)mirror_pixels,
               (unsigned long long)passes, (unsigned long long)pixels, (unsigned long long)rays, (unsigned long long)passed, (unsigned long long)pairs,
               (unsigned long long)hits, (unsigned long long)differ_water, (unsigned long long)differ_other, finite);
    }
    status = 0;
    goto out;
fail:
    fprintf(stderr, "ocean_waves: %s\n", ow_last_error());
out:
    free(rgba); free(ref); free(kinds); free(px); free(linear);
    (void)hipFree(rgba_dev); (void)hipFree(px_dev); (void)hipFree(ref_dev); (void)hipFree(linear_dev);
    ow_radiance_destroy(ctx, radiance);
    ow_sky_destroy(ctx, sky);
    ow_solid_destroy(ctx, solid);
    ow_bodies_destroy(ctx, set);
    ow_mesh_destroy(ctx, mesh);
    ow_destroy(ctx);
    return status;
}

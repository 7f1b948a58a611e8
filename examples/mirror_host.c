/* mirror_host.c -- the sea with crates AND THEIR REFLECTIONS IN THE WATER, from plain C99: sky_light_host.c's scene (the reference scene's
 * three cascades, crates floating on them, a small procedural gradient panorama and its radiance pyramid) seen from low over the water, the
 * frame drawn in the order water, solids, mirror, environment, present -- ow_mesh_draw_async and ow_solid_draw_async with their flat
 * ambient_color set to 0, ow_mirror_apply_async (everything ow_radiance_light_apply does, and the crates' lit colour where a water pixel's
 * mirror ray meets one), ow_environment_apply_async, ow_present_async -- in the context's stream order with no synchronisation in between;
 * the sRGB picture is copied back and written as a binary PPM.  The same records go through ow_radiance_light_apply_async as well, for
 * comparison: only water pixels may differ.
 *   gcc -O2 -std=c99 -Iinclude examples/mirror_host.c -o mirror_host -Lgodotoceanwaves_amd -locean_waves -L/opt/rocm/lib -lamdhip64 \
 *       -Wl,-rpath,$PWD/godotoceanwaves_amd -Wl,-rpath,/opt/rocm/lib -lm && ./mirror_host [out.ppm [width height [steps [map_size [sky_only.ppm [kinds.bin]]]]]]
 * sky_only.ppm: the comparison frame; kinds.bin: one byte a pixel, 0 sky, 1 water, 2 crate.  Prints key=value pairs: the image size, the
 * pixels that show a crate, the pixels that reflect one, the pass's counters, the pixels in which the two frames differ (water, and everything
 * else: 0) and whether every resolved linear colour is finite. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ocean_waves.h"

/* the HIP runtime calls this host makes (libamdhip64, C linkage), declared here because the HIP headers are not C99 */
extern int hipMalloc(void **ptr, size_t bytes);
extern int hipFree(void *ptr);
extern int hipMemcpy(void *dst, const void *src, size_t bytes, int kind);
enum { HIP_DEVICE_TO_HOST = 2, HIP_DEVICE_TO_DEVICE = 3 };

#define CELLS 128
#define CELL 4.0f
#define CRATES 36
#define NX 4
#define NY 2
#define NZ 4
#define PER_CRATE (NX * NY * NZ)
#define SUBSTEPS 4
#define PANO_W 256
#define PANO_H 128

static ow_rigid_body bodies[CRATES];
static ow_hull_point hull[CRATES * PER_CRATE];

/* the panorama: a zenith-to-horizon gradient above, a darker one below, brighter towards the seam (+Z); integers only */
static void make_panorama(unsigned char *p) {
    const int half = PANO_H / 2;
    for (int j = 0; j < PANO_H; ++j)
        for (int i = 0; i < PANO_W; ++i) {
            unsigned char *t = p + 4 * (j * PANO_W + i);
            const int up = j < half, k = up ? j : PANO_H - 1 - j;   /* 0 at a pole .. half - 1 at the horizon */
            const int az = (20 * abs(2 * i - PANO_W)) / PANO_W;
            t[0] = (unsigned char)((up ? 60 + (150 * k) / (half - 1) : 30 + (40 * k) / (half - 1)) + az);
            t[1] = (unsigned char)((up ? 110 + (110 * k) / (half - 1) : 50 + (50 * k) / (half - 1)) + az);
            t[2] = (unsigned char)(up ? 200 + (40 * k) / (half - 1) : 70 + (60 * k) / (half - 1));
            t[3] = 255;
        }
}

static int write_ppm(const char *path, const unsigned char *rgba, int width, int height) {
    FILE *f = fopen(path, "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", path); return 1; }
    fprintf(f, "P6\n%d %d\n255\n", width, height);
    for (size_t i = 0; i < (size_t)width * (size_t)height; ++i) fwrite(rgba + 4 * i, 1, 3, f);
    fclose(f);
    return 0;
}

int main(int argc, char **argv) {
    const char *path = argc > 1 ? argv[1] : "mirror.ppm", *ref_path = argc > 6 ? argv[6] : NULL, *kinds_path = argc > 7 ? argv[7] : NULL;
    const int width = argc > 3 ? atoi(argv[2]) : 320, height = argc > 3 ? atoi(argv[3]) : 200;
    const int steps = argc > 4 ? atoi(argv[4]) : 150, n = argc > 5 ? atoi(argv[5]) : 256, cascades = 3;
    const double dt = 1.0 / 50.0;   /* water.gd:51 */

    ow_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.map_size = n; cfg.num_cascades = cascades; cfg.device_id = -1; cfg.depth = 20.0f;
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
    if (width < 1 || height < 1 || width > OW_RENDER_MAX_SIDE || height > OW_RENDER_MAX_SIDE) { fprintf(stderr, "bad image size\n"); goto fail_quiet; }

    {   /* the sky and its radiance pyramid: six levels from 256 x 128 down to 8 x 4, 64 samples a texel, and the 32 x 16 irradiance */
        static unsigned char panorama[PANO_W * PANO_H * 4];
        make_panorama(panorama);
        if (ow_sky_create(ctx, NULL, panorama, PANO_W, PANO_H, &sky) != OW_OK) goto fail;
        if (ow_radiance_create(ctx, sky, NULL, &radiance) != OW_OK) goto fail;
    }

    {   /* the crates: the states and the voxelised hulls of floating_bodies_host.c, all of one size, and that box as a shape */
        const double size[3] = {2.0, 1.0, 2.0}, rho = 1025.0;
        const double volume = size[0] * size[1] * size[2], mass = 0.5 * rho * volume;
        float corners[8][3];
        static const int32_t quads[6][4] = {{0, 1, 3, 2}, {4, 6, 7, 5}, {0, 4, 5, 1}, {2, 3, 7, 6}, {0, 2, 6, 4}, {1, 5, 7, 3}};   /* -x +x -y +y -z +z */
        int32_t idx[12][3];
        memset(bodies, 0, sizeof bodies);
        memset(hull, 0, sizeof hull);
        for (int b = 0; b < CRATES; ++b) {
            ow_rigid_body *B = &bodies[b];
            B->position[0] = (b % 6 - 2.5) * 6.0; B->position[1] = 0.3; B->position[2] = 10.0 + (b / 6 - 2.5) * 6.0;
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
                        hull[k].local[0] = (float)((i + 0.5) * (size[0] / NX) - size[0] / 2);
                        hull[k].local[1] = (float)((j + 0.5) * (size[1] / NY) - size[1] / 2);
                        hull[k].local[2] = (float)((l + 0.5) * (size[2] / NZ) - size[2] / 2);
                        hull[k].volume = (float)(volume / PER_CRATE);
                        hull[k].half_height = (float)(size[1] / NY / 2);
                        hull[k].body = b;
                    }
        }
        if (ow_bodies_create(ctx, bodies, CRATES, hull, CRATES * PER_CRATE, &set) != OW_OK) goto fail;
        for (int v = 0; v < 8; ++v) {   /* corner 4 ix + 2 iy + iz; every face counter-clockwise seen from outside */
            corners[v][0] = (float)((v & 4 ? 0.5 : -0.5) * size[0]);
            corners[v][1] = (float)((v & 2 ? 0.5 : -0.5) * size[1]);
            corners[v][2] = (float)((v & 1 ? 0.5 : -0.5) * size[2]);
        }
        for (int q = 0; q < 6; ++q) {
            idx[2 * q][0] = quads[q][0]; idx[2 * q][1] = quads[q][1]; idx[2 * q][2] = quads[q][2];
            idx[2 * q + 1][0] = quads[q][0]; idx[2 * q + 1][1] = quads[q][2]; idx[2 * q + 1][2] = quads[q][3];
        }
        if (ow_solid_create(ctx, &corners[0][0], 8, &idx[0][0], 12, &solid) != OW_OK) goto fail;
    }

    {   /* the grid: (CELLS + 1)^2 vertices around the node's origin, two triangles a cell */
        const int32_t num_vertices = (CELLS + 1) * (CELLS + 1), num_triangles = 2 * CELLS * CELLS;
        float *xyz = (float *)malloc((size_t)num_vertices * 3 * sizeof(float));
        int32_t *idx = (int32_t *)malloc((size_t)num_triangles * 3 * sizeof(int32_t));
        if (!xyz || !idx) { fprintf(stderr, "out of memory\n"); goto fail_quiet; }
        for (int r = 0; r <= CELLS; ++r)
            for (int c = 0; c <= CELLS; ++c) {
                float *v = xyz + 3 * ((size_t)r * (CELLS + 1) + c);
                v[0] = (float)c * CELL - 0.5f * CELLS * CELL; v[1] = 0.0f; v[2] = (float)r * CELL - 0.5f * CELLS * CELL;
            }
        for (int r = 0; r < CELLS; ++r)
            for (int c = 0; c < CELLS; ++c) {
                const int32_t a = r * (CELLS + 1) + c, b = a + 1, d = a + CELLS + 1, e = d + 1;
                int32_t *t = idx + 6 * ((size_t)r * CELLS + c);
                t[0] = a; t[1] = d; t[2] = b; t[3] = b; t[4] = d; t[5] = e;
            }
        const ow_status st = ow_mesh_create(ctx, xyz, num_vertices, idx, num_triangles, &mesh);
        free(xyz); free(idx);
        if (st != OW_OK) goto fail;
    }

    ow_camera cam;
    memset(&cam, 0, sizeof cam);
    {   /* 3.5 m over the water, 12 m in front of the first row of crates, looking along +z and 8 degrees down: the crates stand over their images */
        static const float basis[9] = {-1.0f, 0.0f, 0.0f, 0.0f, 0.990268f, 0.139173f, 0.0f, 0.139173f, -0.990268f};
        memcpy(cam.basis, basis, sizeof basis);
        cam.position[0] = 0.0f; cam.position[1] = 3.5f; cam.position[2] = -17.0f;
    }
    cam.fov_y_degrees = 60.0f;
    cam.max_distance = 4000.0f;
    cam.width = width; cam.height = height;
    const float origin[3] = {ceilf(cam.position[0] / CELL) * CELL, 0.0f, ceilf(cam.position[2] / CELL) * CELL};   /* main.gd:34-37 */

    ow_mesh_options opts;
    ow_mesh_options_default(&opts);
    opts.query_flags = OW_QUERY_DISTANCE_FALLOFF;   /* water.gdshader:29, around CAMERA_POSITION_WORLD.xz */
    opts.falloff_center_xz[0] = cam.position[0];
    opts.falloff_center_xz[1] = cam.position[2];
    opts.flags = OW_MESH_CULL_BACK;
    opts.ambient_color[0] = opts.ambient_color[1] = opts.ambient_color[2] = 0.0f;   /* the sky lights the frame: no flat ambient */
    ow_solid_options sopts;
    ow_solid_options_default(&sopts);
    sopts.ambient_color[0] = sopts.ambient_color[1] = sopts.ambient_color[2] = 0.0f;
    ow_mirror_options mo;
    ow_mirror_options_init(&mo);                    /* the draw's colour and sun; its ambient as the draw has it: 0 */
    mo.ambient_color[0] = mo.ambient_color[1] = mo.ambient_color[2] = 0.0f;

    const size_t count = (size_t)width * (size_t)height;
    if (hipMalloc(&rgba_dev, count * 4) || hipMalloc(&linear_dev, count * 16) || hipMalloc(&px_dev, count * sizeof(ow_render_pixel)) ||
        hipMalloc(&ref_dev, count * sizeof(ow_render_pixel))) { fprintf(stderr, "hipMalloc failed\n"); goto fail_quiet; }
    rgba = (unsigned char *)malloc(count * 4);
    ref = (unsigned char *)malloc(count * 4);
    kinds = (unsigned char *)malloc(count);
    linear = (float *)malloc(count * 16);
    px = (ow_render_pixel *)malloc(count * sizeof(ow_render_pixel));
    if (!rgba || !ref || !kinds || !px || !linear) { fprintf(stderr, "out of memory\n"); goto fail_quiet; }

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
    if (ow_solid_draw_async(ctx, solid, set, 0, CRATES, &cam, &sopts, (ow_render_pixel *)px_dev, NULL) != OW_OK) goto fail;
    if (ow_sync(ctx) != OW_OK) goto fail;
    if (hipMemcpy(ref_dev, px_dev, count * sizeof(ow_render_pixel), HIP_DEVICE_TO_DEVICE)) { fprintf(stderr, "hipMemcpy failed\n"); goto fail_quiet; }
    if (ow_radiance_light_apply_async(ctx, radiance, &cam, NULL, (ow_render_pixel *)ref_dev) != OW_OK) goto fail;   /* main.tscn:16-24 */
    if (ow_environment_apply_async(ctx, sky, &cam, NULL, (ow_render_pixel *)ref_dev) != OW_OK) goto fail;
    if (ow_present_async(ctx, &cam, &po, (const ow_render_pixel *)ref_dev, rgba_dev, NULL) != OW_OK) goto fail;
    if (ow_sync(ctx) != OW_OK) goto fail;
    if (hipMemcpy(ref, rgba_dev, count * 4, HIP_DEVICE_TO_HOST)) { fprintf(stderr, "hipMemcpy failed\n"); goto fail_quiet; }
    if (ow_mirror_apply_async(ctx, radiance, solid, set, 0, CRATES, &cam, &mo, (ow_render_pixel *)px_dev, NULL) != OW_OK) goto fail;
    if (ow_environment_apply_async(ctx, sky, &cam, NULL, (ow_render_pixel *)px_dev) != OW_OK) goto fail;   /* main.tscn:22-34 */
    if (ow_present_async(ctx, &cam, &po, (const ow_render_pixel *)px_dev, rgba_dev, (float *)linear_dev) != OW_OK) goto fail;
    if (ow_sync(ctx) != OW_OK) goto fail;
    if (hipMemcpy(rgba, rgba_dev, count * 4, HIP_DEVICE_TO_HOST) || hipMemcpy(linear, linear_dev, count * 16, HIP_DEVICE_TO_HOST) ||
        hipMemcpy(px, px_dev, count * sizeof(ow_render_pixel), HIP_DEVICE_TO_HOST)) {
        fprintf(stderr, "hipMemcpy failed\n");
        goto fail_quiet;
    }
    if (write_ppm(path, rgba, width, height)) goto fail_quiet;
    if (ref_path && write_ppm(ref_path, ref, width, height)) goto fail_quiet;

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
        if (kinds_path) {
            FILE *f = fopen(kinds_path, "wb");
            if (!f) { fprintf(stderr, "cannot write %s\n", kinds_path); goto fail_quiet; }
            fwrite(kinds, 1, count, f);
            fclose(f);
        }
        if (ow_mirror_stats(ctx, &passes, &pixels, &rays, &passed, &pairs, &hits) != OW_OK) goto fail;
        printf("file=%s width=%d height=%d steps=%d crates=%d water_pixels=%llu crate_pixels=%llu mirror_pixels=%llu passes=%llu pixels=%llu rays_cast=%llu "
               "sphere_tests_passed=%llu pairs_tested=%llu rays_hit=%llu differing_water_pixels=%llu differing_other_pixels=%llu finite=%d\n",
               path, width, height, steps, CRATES, (unsigned long long)water_pixels, (unsigned long long)crate_pixels, (unsigned long long)mirror_pixels,
               (unsigned long long)passes, (unsigned long long)pixels, (unsigned long long)rays, (unsigned long long)passed, (unsigned long long)pairs,
               (unsigned long long)hits, (unsigned long long)differ_water, (unsigned long long)differ_other, finite);
    }
    free(rgba); free(ref); free(kinds); free(px); free(linear);
    (void)hipFree(rgba_dev); (void)hipFree(px_dev); (void)hipFree(ref_dev); (void)hipFree(linear_dev);
    ow_radiance_destroy(ctx, radiance);
    ow_sky_destroy(ctx, sky);
    ow_solid_destroy(ctx, solid);
    ow_bodies_destroy(ctx, set);
    ow_mesh_destroy(ctx, mesh);
    ow_destroy(ctx);
    return 0;
fail:
    fprintf(stderr, "ocean_waves: %s\n", ow_last_error());
fail_quiet:
    free(rgba); free(ref); free(kinds); free(px); free(linear);
    (void)hipFree(rgba_dev); (void)hipFree(px_dev); (void)hipFree(ref_dev); (void)hipFree(linear_dev);
    ow_radiance_destroy(ctx, radiance);
    ow_sky_destroy(ctx, sky);
    ow_solid_destroy(ctx, solid);
    ow_bodies_destroy(ctx, set);
    ow_mesh_destroy(ctx, mesh);
    ow_destroy(ctx);
    return 1;
}

/* mist_host.c -- the sea, 36 crates and THE SHAFTS THEIR SHADOWS CUT INTO THE SEA MIST, from plain C99: the reference scene's three
 * cascades, the crates of shadow_host.c floating on them, a shadow map of the crates from the scene's low sun, and the frame drawn in the
 * order water, solids, shadows, environment, mist, present -- ow_mesh_draw_async, ow_solid_draw_async, ow_shadow_map_begin / _cast,
 * ow_shadow_apply_async, ow_environment_apply_async, ow_mist_apply_async (the map's casters shadow the mist), ow_present_async -- in the
 * context's stream order with no synchronisation in between; the sRGB picture is copied back and written as a binary PPM.
 *   gcc -O2 -std=c99 -Iinclude examples/mist_host.c -o mist_host -Lgodotoceanwaves_amd -locean_waves -L/opt/rocm/lib -lamdhip64 \
 *       -Wl,-rpath,$PWD/godotoceanwaves_amd -Wl,-rpath,/opt/rocm/lib -lm && ./mist_host [out.ppm [width height [steps [map_size [downsample [shadow_size [slices]]]]]]]
 * width x height is the size of the PPM; the records are drawn at downsample (1 .. 4, default 2) times that.  Prints key=value pairs: the
 * image size, the record size, the shadow map's size, the mist pass's counters, the pixels it marked and whether every resolved linear
 * colour is finite. */
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
enum { HIP_DEVICE_TO_HOST = 2 };

#define CELLS 128
#define CELL 4.0f
#define CRATES 36
#define NX 4
#define NY 2
#define NZ 4
#define PER_CRATE (NX * NY * NZ)
#define SUBSTEPS 4
#define SHADOW_SIZE 1024

static ow_rigid_body bodies[CRATES];
static ow_hull_point hull[CRATES * PER_CRATE];

int main(int argc, char **argv) {
    const char *path = argc > 1 ? argv[1] : "mist.ppm";
    const int out_width = argc > 3 ? atoi(argv[2]) : 320, out_height = argc > 3 ? atoi(argv[3]) : 200, down = argc > 6 ? atoi(argv[6]) : 2;
    const int steps = argc > 4 ? atoi(argv[4]) : 150, n = argc > 5 ? atoi(argv[5]) : 256, cascades = 3;
    const double dt = 1.0 / 50.0;   /* water.gd:51 */
    const int shadow_size = argc > 7 ? atoi(argv[7]) : SHADOW_SIZE, slices = argc > 8 ? atoi(argv[8]) : 0;

    ow_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.map_size = n; cfg.num_cascades = cascades; cfg.device_id = -1; cfg.depth = 20.0f;
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
    if (down < 1 || down > OW_PRESENT_MAX_DOWNSAMPLE || out_width < 1 || out_height < 1 || out_width > OW_RENDER_MAX_SIDE / down ||
        out_height > OW_RENDER_MAX_SIDE / down) { fprintf(stderr, "bad image size\n"); goto fail_quiet; }
    const int width = out_width * down, height = out_height * down;   /* the records */

    if (ow_shadow_map_create(ctx, shadow_size, &shadow) != OW_OK) goto fail;

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
        if (!xyz || !idx) { fprintf(stderr, "out of memory\n"); free(xyz); free(idx); goto fail_quiet; }
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
    {   /* main.tscn:120 */
        static const float basis[9] = {-0.996195f, -0.0151344f, 0.0858316f, 0.0f, 0.984807f, 0.173648f, -0.0871557f, 0.172987f, -0.981061f};
        memcpy(cam.basis, basis, sizeof basis);
        cam.position[0] = 0.0f; cam.position[1] = 10.0f; cam.position[2] = -25.0f;
    }
    cam.fov_y_degrees = 75.0f;
    cam.max_distance = 4000.0f;
    cam.width = width; cam.height = height;
    const float origin[3] = {ceilf(cam.position[0] / CELL) * CELL, 0.0f, ceilf(cam.position[2] / CELL) * CELL};   /* main.gd:34-37 */

    ow_mesh_options opts;
    ow_mesh_options_default(&opts);
    opts.query_flags = OW_QUERY_DISTANCE_FALLOFF;   /* water.gdshader:29, around CAMERA_POSITION_WORLD.xz */
    opts.falloff_center_xz[0] = cam.position[0];
    opts.falloff_center_xz[1] = cam.position[2];
    opts.flags = OW_MESH_CULL_BACK;

    const size_t count = (size_t)width * (size_t)height, out_count = (size_t)out_width * (size_t)out_height;
    if (hipMalloc(&rgba_dev, out_count * 4) || hipMalloc(&linear_dev, out_count * 16) || hipMalloc(&px_dev, count * sizeof(ow_render_pixel))) { fprintf(stderr, "hipMalloc failed\n"); goto fail_quiet; }

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
    if (ow_solid_draw_async(ctx, solid, set, 0, CRATES, &cam, NULL, (ow_render_pixel *)px_dev, NULL) != OW_OK) goto fail;
    if (ow_shadow_map_begin(ctx, shadow, &frame) != OW_OK) goto fail;
    if (ow_shadow_map_cast(ctx, shadow, solid, set, 0, CRATES) != OW_OK) goto fail;   /* the poses stay on the device */
    if (ow_shadow_apply_async(ctx, shadow, &cam, &sho, (ow_render_pixel *)px_dev, NULL) != OW_OK) goto fail;
    if (ow_environment_apply_async(ctx, NULL, &cam, NULL, (ow_render_pixel *)px_dev) != OW_OK) goto fail;   /* main.tscn:22-34 */
    if (ow_mist_apply_async(ctx, shadow, &cam, &mo, (ow_render_pixel *)px_dev, NULL) != OW_OK) goto fail;
    if (ow_present_async(ctx, &cam, &po, (const ow_render_pixel *)px_dev, rgba_dev, (float *)linear_dev) != OW_OK) goto fail;
    if (ow_sync(ctx) != OW_OK) goto fail;

    rgba = (unsigned char *)malloc(out_count * 4);
    linear = (float *)malloc(out_count * 16);
    px = (ow_render_pixel *)malloc(count * sizeof(ow_render_pixel));
    if (!rgba || !px || !linear) { fprintf(stderr, "out of memory\n"); goto fail_quiet; }
    if (hipMemcpy(rgba, rgba_dev, out_count * 4, HIP_DEVICE_TO_HOST) || hipMemcpy(linear, linear_dev, out_count * 16, HIP_DEVICE_TO_HOST) ||
        hipMemcpy(px, px_dev, count * sizeof(ow_render_pixel), HIP_DEVICE_TO_HOST)) {
        fprintf(stderr, "hipMemcpy failed\n");
        goto fail_quiet;
    }
    FILE *f = fopen(path, "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", path); goto fail_quiet; }
    fprintf(f, "P6\n%d %d\n255\n", out_width, out_height);
    for (size_t i = 0; i < out_count; ++i) fwrite(rgba + 4 * i, 1, 3, f);
    fclose(f);

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
               path, out_width, out_height, down, width, height, steps, CRATES, shadow_size, (unsigned long long)passes, (unsigned long long)pixels,
               (unsigned long long)fetched, (unsigned long long)shadowed, (unsigned long long)misted, (unsigned long long)crate_pixels, finite);
    }
    free(rgba); free(px); free(linear);
    (void)hipFree(rgba_dev); (void)hipFree(px_dev); (void)hipFree(linear_dev);
    ow_shadow_map_destroy(ctx, shadow);
    ow_solid_destroy(ctx, solid);
    ow_bodies_destroy(ctx, set);
    ow_mesh_destroy(ctx, mesh);
    ow_destroy(ctx);
    return 0;
fail:
    fprintf(stderr, "ocean_waves: %s\n", ow_last_error());
fail_quiet:
    free(rgba); free(px); free(linear);
    (void)hipFree(rgba_dev); (void)hipFree(px_dev); (void)hipFree(linear_dev);
    ow_shadow_map_destroy(ctx, shadow);
    ow_solid_destroy(ctx, solid);
    ow_bodies_destroy(ctx, set);
    ow_mesh_destroy(ctx, mesh);
    ow_destroy(ctx);
    return 1;
}

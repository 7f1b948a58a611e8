/* mesh_host.c -- the water as the reference draws it, a displaced mesh, from plain C99: creates a context, ticks it, uploads a grid mesh it
 * generates itself, draws the reference scene's camera with ow_mesh_draw and writes a binary PPM.
 *   gcc -O2 -std=c99 -Iinclude examples/mesh_host.c -o mesh_host -Lgodotoceanwaves_amd -locean_waves \
 *       -Wl,-rpath,$PWD/godotoceanwaves_amd -Wl,-rpath-link,/opt/rocm/lib -lm && ./mesh_host [out.ppm [width height [ticks [map_size]]]]
 * The scene is render_host.c's (main.tscn's camera and sun, mat_water.tres, water.gd's colours, the three cascades).  The mesh is a flat
 * grid of 128 x 128 cells of 4 m, wound counter-clockwise seen from above, put where main.gd:34-37 puts the clipmap for the low mesh
 * quality: ceil(camera.xz / 4) * 4.  The shader's distance falloff is centred on the camera and back faces are culled, as Godot draws this
 * material.  Prints key=value pairs: the image size, the mesh, the share of pixels the mesh covers and whether every record is finite. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ocean_waves.h"

#define CELLS 128
#define CELL 4.0f

int main(int argc, char **argv) {
    const char *path = argc > 1 ? argv[1] : "mesh.ppm";
    const int width = argc > 3 ? atoi(argv[2]) : 320, height = argc > 3 ? atoi(argv[3]) : 200;
    const int ticks = argc > 4 ? atoi(argv[4]) : 10, n = argc > 5 ? atoi(argv[5]) : 256, cascades = 3;
    const double dt = 1.0 / 50.0;   /* water.gd:51 */

    ow_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.map_size = n; cfg.num_cascades = cascades; cfg.device_id = -1; cfg.depth = 20.0f;
    ow_context *ctx = NULL;
    ow_mesh *mesh = NULL;
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
    for (int t = 0; t < ticks; ++t)
        if (ow_update_all(ctx, dt, par, cascades) != OW_OK) goto fail;

    /* the grid: (CELLS + 1)^2 vertices around the node's origin, two triangles a cell */
    const int32_t num_vertices = (CELLS + 1) * (CELLS + 1), num_triangles = 2 * CELLS * CELLS;
    float *xyz = (float *)malloc((size_t)num_vertices * 3 * sizeof(float));
    int32_t *idx = (int32_t *)malloc((size_t)num_triangles * 3 * sizeof(int32_t));
    if (!xyz || !idx) { fprintf(stderr, "out of memory\n"); return 1; }
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
    if (ow_mesh_create(ctx, xyz, num_vertices, idx, num_triangles, &mesh) != OW_OK) goto fail;
    free(xyz); free(idx);

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

    if (width < 1 || height < 1 || width > OW_RENDER_MAX_SIDE || height > OW_RENDER_MAX_SIDE) { fprintf(stderr, "bad image size\n"); goto fail_quiet; }
    const size_t count = (size_t)width * (size_t)height;
    unsigned char *rgba = (unsigned char *)malloc(count * 4);
    ow_render_pixel *px = (ow_render_pixel *)malloc(count * sizeof(ow_render_pixel));
    if (!rgba || !px) { fprintf(stderr, "out of memory\n"); return 1; }
    if (ow_mesh_draw(ctx, mesh, &cam, origin, &map_scales[0][0], cascades, &opts, rgba, px) != OW_OK) goto fail;
    uint64_t skipped = 0, culled = 0, per_lane = 0, cooperative = 0;
    if (ow_mesh_stats(ctx, mesh, NULL, &skipped, &culled, &per_lane, &cooperative) != OW_OK) goto fail;

    FILE *f = fopen(path, "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", path); return 1; }
    fprintf(f, "P6\n%d %d\n255\n", width, height);
    for (size_t i = 0; i < count; ++i) fwrite(rgba + 4 * i, 1, 3, f);
    fclose(f);

    {
        size_t hits = 0;
        int finite = 1;
        for (size_t i = 0; i < count; ++i) {
            finite &= isfinite(px[i].t) && isfinite(px[i].fresnel) && isfinite(px[i].specular);
            for (int k = 0; k < 3; ++k) finite &= isfinite(px[i].color[k]) && isfinite(px[i].diffuse[k]) && isfinite(px[i].normal[k]);
            if (px[i].status & OW_RAY_HIT) ++hits;
        }
        printf("file=%s width=%d height=%d ticks=%d triangles=%d per_lane=%llu cooperative=%llu culled=%llu hit_share=%.4f finite=%d\n", path, width,
               height, ticks, (int)num_triangles, (unsigned long long)per_lane, (unsigned long long)cooperative, (unsigned long long)(culled + skipped),
               (double)hits / (double)count, finite);
    }
    free(rgba); free(px);
    ow_mesh_destroy(ctx, mesh);
    ow_destroy(ctx);
    return 0;
fail:
    fprintf(stderr, "ocean_waves: %s\n", ow_last_error());
fail_quiet:
    ow_mesh_destroy(ctx, mesh);
    ow_destroy(ctx);
    return 1;
}

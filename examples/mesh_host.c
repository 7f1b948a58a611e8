/* mesh_host.c -- the water as the reference draws it, a displaced mesh, from plain C99: creates a context, ticks it, uploads a grid mesh it
 * generates itself, draws the reference scene's camera with ow_mesh_draw and writes a binary PPM.
 *   gcc -O2 -std=c99 -Iinclude examples/mesh_host.c -o mesh_host -Lgodotoceanwaves_amd -locean_waves \
 *       -Wl,-rpath,$PWD/godotoceanwaves_amd -Wl,-rpath-link,/opt/rocm/lib -lm && ./mesh_host [out.ppm [width height [ticks [map_size]]]]
 * The scene is render_host.c's (main.tscn's camera and sun, mat_water.tres, water.gd's colours, the three cascades).  The mesh is scene.h's:
 * a flat grid of 128 x 128 cells of 4 m, wound counter-clockwise seen from above, put where main.gd:34-37 puts the clipmap for the low mesh
 * quality: ceil(camera.xz / 4) * 4.  The shader's distance falloff is centred on the camera and back faces are culled, as Godot draws this
 * material.  Prints key=value pairs: the image size, the mesh, the share of pixels the mesh covers and whether every record is finite. */
#include "scene.h"

int main(int argc, char **argv) {
    const char *path = argc > 1 ? argv[1] : "mesh.ppm";
    const int width = argc > 3 ? atoi(argv[2]) : 320, height = argc > 3 ? atoi(argv[3]) : 200;
    const int ticks = scene_arg(argc, argv, 4, 10), n = scene_arg(argc, argv, 5, 256), cascades = SCENE_CASCADES;
    const double dt = 1.0 / 50.0;   /* water.gd:51 */
    int status = 1;

    ow_config cfg;
    scene_config(&cfg, n);
    ow_context *ctx = NULL;
    ow_mesh *mesh = NULL;
    unsigned char *rgba = NULL;
    ow_render_pixel *px = NULL;
    if (ow_create(&cfg, &ctx) != OW_OK) { fprintf(stderr, "ow_create: %s\n", ow_last_error()); return 1; }

    ow_cascade_params par[SCENE_CASCADES];
    float map_scales[SCENE_CASCADES][4];
    scene_cascades(par, map_scales);
    for (int t = 0; t < ticks; ++t)
        if (ow_update_all(ctx, dt, par, cascades) != OW_OK) goto fail;

    if (scene_grid_create(ctx, SCENE_CELLS, SCENE_CELL, &mesh)) goto out;

    ow_camera cam;
    float origin[3];
    scene_camera(&cam, width, height);
    scene_clipmap_origin(&cam, SCENE_CELL, origin);
    ow_mesh_options opts;
    scene_mesh_options(&opts, &cam);

    if (scene_bad_size(width, height, 1)) goto out;
    const size_t count = (size_t)width * (size_t)height;
    rgba = (unsigned char *)malloc(count * 4);
    px = (ow_render_pixel *)malloc(count * sizeof(ow_render_pixel));
    if (!rgba || !px) { fprintf(stderr, "out of memory\n"); goto out; }
    if (ow_mesh_draw(ctx, mesh, &cam, origin, &map_scales[0][0], cascades, &opts, rgba, px) != OW_OK) goto fail;
    uint64_t skipped = 0, culled = 0, per_lane = 0, cooperative = 0;
    if (ow_mesh_stats(ctx, mesh, NULL, &skipped, &culled, &per_lane, &cooperative) != OW_OK) goto fail;
    if (scene_write_ppm(path, rgba, width, height)) goto out;

    {
        size_t hits = 0;
        int finite = 1;
        for (size_t i = 0; i < count; ++i) {
            finite &= isfinite(px[i].t) && isfinite(px[i].fresnel) && isfinite(px[i].specular);
            for (int k = 0; k < 3; ++k) finite &= isfinite(px[i].color[k]) && isfinite(px[i].diffuse[k]) && isfinite(px[i].normal[k]);
            if (px[i].status & OW_RAY_HIT) ++hits;
        }
        printf("file=%s width=%d height=%d ticks=%d triangles=%d per_lane=%llu cooperative=%llu culled=%llu hit_share=%.4f finite=%d\n", path, width,
               height, ticks, 2 * SCENE_CELLS * SCENE_CELLS, (unsigned long long)per_lane, (unsigned long long)cooperative, (unsigned long long)(culled + skipped),
               (double)hits / (double)count, finite);
    }
    status = 0;
    goto out;
fail:
    fprintf(stderr, "ocean_waves: %s\n", ow_last_error());
out:
    free(rgba); free(px);
    ow_mesh_destroy(ctx, mesh);
    ow_destroy(ctx);
    return status;
}

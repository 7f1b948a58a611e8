/* render_host.c -- a picture of the water from plain C99, on a machine without a rasteriser: creates a context, ticks it, renders the
 * reference scene's camera with ow_render_view and writes a binary PPM.
 *   gcc -O2 -std=c99 -Iinclude examples/render_host.c -o render_host -Lgodotoceanwaves_amd -locean_waves \
 *       -Wl,-rpath,$PWD/godotoceanwaves_amd -Wl,-rpath-link,/opt/rocm/lib && ./render_host [out.ppm [width height [ticks [map_size]]]]
 * The scene's values are the reference's settings, restated as numbers:
 *   main.tscn:119-120   the camera's Transform3D (at (0, 10, -25), looking towards +z, ten degrees down); Camera3D's default fov 75 and far 4000
 *   main.tscn:112-113   the sun's Transform3D: the light comes from its +Z axis
 *   mat_water.tres:8-9  roughness 0.65, normal_strength 1
 *   water.gd:14-18      water_color (0.1, 0.15, 0.18) and foam_color (0.73, 0.67, 0.62), sRGB, converted to linear
 *   main.tscn:43-83     the three cascades
 * ow_render_options_default holds the material and the sun; the shader's distance falloff is centred on the camera, as the reference
 * renders.  The PPM holds the RGBA8 words' R, G, B as they are (linear, no transfer curve).  Prints key=value pairs: the image size, the
 * share of pixels that hit the water, the mean colour of those and whether every record is finite. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ocean_waves.h"

int main(int argc, char **argv) {
    const char *path = argc > 1 ? argv[1] : "water.ppm";
    const int width = argc > 3 ? atoi(argv[2]) : 320, height = argc > 3 ? atoi(argv[3]) : 200;
    const int ticks = argc > 4 ? atoi(argv[4]) : 10, n = argc > 5 ? atoi(argv[5]) : 256, cascades = 3;
    const double dt = 1.0 / 50.0;   /* water.gd:51 */

    ow_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.map_size = n; cfg.num_cascades = cascades; cfg.device_id = -1; cfg.depth = 20.0f;
    ow_context *ctx = NULL;
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

    ow_render_options opts;
    ow_render_options_default(&opts);
    opts.raycast.query.flags = OW_QUERY_DISTANCE_FALLOFF;   /* water.gdshader:29, around CAMERA_POSITION_WORLD.xz */
    opts.raycast.query.falloff_center_xz[0] = cam.position[0];
    opts.raycast.query.falloff_center_xz[1] = cam.position[2];

    if (width < 1 || height < 1 || width > OW_RENDER_MAX_SIDE || height > OW_RENDER_MAX_SIDE) { fprintf(stderr, "bad image size\n"); ow_destroy(ctx); return 1; }
    const size_t count = (size_t)width * (size_t)height;
    unsigned char *rgba = (unsigned char *)malloc(count * 4);
    ow_render_pixel *px = (ow_render_pixel *)malloc(count * sizeof(ow_render_pixel));
    if (!rgba || !px) { fprintf(stderr, "out of memory\n"); return 1; }
    if (ow_render_view(ctx, &cam, &map_scales[0][0], cascades, &opts, rgba, px) != OW_OK) goto fail;

    FILE *f = fopen(path, "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", path); return 1; }
    fprintf(f, "P6\n%d %d\n255\n", width, height);
    for (size_t i = 0; i < count; ++i) fwrite(rgba + 4 * i, 1, 3, f);
    fclose(f);

    {
        size_t hits = 0;
        int finite = 1;
        double mean[3] = {0.0, 0.0, 0.0};
        for (size_t i = 0; i < count; ++i) {
            finite &= isfinite(px[i].t) && isfinite(px[i].fresnel) && isfinite(px[i].specular);
            for (int k = 0; k < 3; ++k) finite &= isfinite(px[i].color[k]) && isfinite(px[i].diffuse[k]) && isfinite(px[i].normal[k]);
            if (px[i].status & OW_RAY_HIT) {
                ++hits;
                for (int k = 0; k < 3; ++k) mean[k] += px[i].color[k];
            }
        }
        for (int k = 0; k < 3; ++k) mean[k] /= hits ? (double)hits : 1.0;
        printf("file=%s width=%d height=%d ticks=%d hit_share=%.4f mean_color=%.4f,%.4f,%.4f finite=%d\n", path, width, height, ticks,
               (double)hits / (double)count, mean[0], mean[1], mean[2], finite);
    }
    free(rgba); free(px);
    ow_destroy(ctx);
    return 0;
fail:
    fprintf(stderr, "ocean_waves: %s\n", ow_last_error());
    ow_destroy(ctx);
    return 1;
}

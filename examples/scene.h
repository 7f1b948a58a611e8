/* scene.h -- what the example programs share, each piece once: the reference scene as numbers (its three cascades, its camera, the clip-map
 * grid), the picture examples' crates, their procedural sky and spray textures, and the plumbing every host needs (the HIP runtime's C
 * declarations, a PPM writer, argument reading).  Example scaffolding, NOT part of the ABI: header-only C99 (and C++17) of static inline
 * functions and constants, no storage, included as "scene.h" from the file next to it, so the one-line compile commands in the examples'
 * comments need nothing added.  The generators that only fill arrays (crates, box, grid, panorama, textures) call nothing of the library.
 * The FP64 and FP32 expressions are written as the pictures were recorded with them: tests/test_example_scene.py holds tests/scenes.py to
 * them byte for byte, and the pictures are compared by byte, so their shape is not to be "simplified". */
#ifndef OCEAN_WAVES_EXAMPLES_SCENE_H
#define OCEAN_WAVES_EXAMPLES_SCENE_H

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ocean_waves.h"

#ifdef __cplusplus
extern "C" {
#endif
/* the HIP runtime calls the hosts make (libamdhip64, C linkage), declared here because the HIP headers are not C99 */
extern int hipMalloc(void **ptr, size_t bytes);
extern int hipFree(void *ptr);
extern int hipMemcpy(void *dst, const void *src, size_t bytes, int kind);
extern int hipMemcpyAsync(void *dst, const void *src, size_t bytes, int kind, void *stream);
extern int hipStreamCreate(void **stream);
extern int hipStreamDestroy(void *stream);
#ifdef __cplusplus
}
#endif
enum { HIP_HOST_TO_DEVICE = 1, HIP_DEVICE_TO_HOST = 2, HIP_DEVICE_TO_DEVICE = 3 };

enum {
    SCENE_CASCADES = 3,                                        /* main.tscn:43-83 */
    SCENE_CELLS = 128,                                         /* the clip-map grid of the low mesh quality: 128 x 128 cells ... */
    SCENE_CRATES = 36, SCENE_NX = 4, SCENE_NY = 2, SCENE_NZ = 4, SCENE_PER_CRATE = SCENE_NX * SCENE_NY * SCENE_NZ,
    SCENE_BOX_VERTICES = 8, SCENE_BOX_TRIANGLES = 12,
    SCENE_PANO_W = 256, SCENE_PANO_H = 128,                    /* the panorama */
    SCENE_TEX = 64                                             /* the side of the two spray textures */
};
#define SCENE_CELL 4.0f                                        /* ... of 4 m */
#define SCENE_CRATE_SIZE {2.0, 1.0, 2.0}                       /* metres */

static inline int scene_arg(int argc, char **argv, int k, int fallback) { return argc > k ? atoi(argv[k]) : fallback; }

/* the context every example creates: map_size^2 texels, the three cascades, the current device, the scene's depth */
static inline void scene_config(ow_config *cfg, int map_size) {
    memset(cfg, 0, sizeof *cfg);
    cfg->map_size = map_size; cfg->num_cascades = SCENE_CASCADES; cfg->device_id = -1; cfg->depth = 20.0f;
}

/* cascade i's seeds and start time, as water.gd:31-32 assigns them */
static inline void scene_cascade_start(ow_cascade_params *p, int i) {
    p->spectrum_seed[0] = 1000 + 17 * i; p->spectrum_seed[1] = -2000 + 31 * i;
    p->time = 120.0 + 3.14159265358979323846 * i;
}

/* the three cascades of the reference's main.tscn and what the water shader scales their maps by (water.gd:105-109) */
static inline void scene_cascades(ow_cascade_params par[SCENE_CASCADES], float map_scales[SCENE_CASCADES][4]) {
    static const float tile[3] = {88.0f, 57.0f, 16.0f}, wind[3] = {10.0f, 5.0f, 20.0f}, dir[3] = {20.0f, 15.0f, 20.0f};
    static const float fetch[3] = {150.0f, 150.0f, 550.0f}, spread[3] = {0.2f, 0.4f, 0.4f}, whitecap[3] = {0.5f, 0.5f, 0.25f}, foam[3] = {8.0f, 0.0f, 3.0f};
    for (int i = 0; i < SCENE_CASCADES; ++i) {
        ow_cascade_params_default(&par[i]);
        par[i].tile_length[0] = par[i].tile_length[1] = tile[i];
        par[i].wind_speed = wind[i]; par[i].wind_direction = dir[i]; par[i].fetch_length = fetch[i];
        par[i].spread = spread[i]; par[i].whitecap = whitecap[i]; par[i].foam_amount = foam[i];
        scene_cascade_start(&par[i], i);
        map_scales[i][0] = map_scales[i][1] = 1.0f / tile[i];
        map_scales[i][2] = (float)par[i].displacement_scale;
        map_scales[i][3] = (float)par[i].normal_scale;
    }
}

/* the crates of the picture examples: boxes of 2 x 1 x 2 m of half the water's density on a 6 x 6 grid 6 m apart in front of the camera,
 * dropped from 0.3 m, each voxelised into 4 x 2 x 4 hull points; bodies[SCENE_CRATES], hull[SCENE_CRATES * SCENE_PER_CRATE] */
static inline void scene_crates(ow_rigid_body *bodies, ow_hull_point *hull) {
    const double size[3] = SCENE_CRATE_SIZE, rho = 1025.0;
    const double volume = size[0] * size[1] * size[2], mass = 0.5 * rho * volume;
    memset(bodies, 0, SCENE_CRATES * sizeof *bodies);
    memset(hull, 0, SCENE_CRATES * SCENE_PER_CRATE * sizeof *hull);
    for (int b = 0; b < SCENE_CRATES; ++b) {
        ow_rigid_body *B = &bodies[b];
        B->position[0] = (b % 6 - 2.5) * 6.0; B->position[1] = 0.3; B->position[2] = 10.0 + (b / 6 - 2.5) * 6.0;
        B->orientation[3] = 1.0;
        B->mass = mass;
        B->inverse_inertia[0] = 12.0 / (mass * (size[1] * size[1] + size[2] * size[2]));
        B->inverse_inertia[1] = 12.0 / (mass * (size[0] * size[0] + size[2] * size[2]));
        B->inverse_inertia[2] = 12.0 / (mass * (size[0] * size[0] + size[1] * size[1]));
        B->linear_drag = 3.0f; B->quadratic_drag = 0.5f;
        B->point_offset = b * SCENE_PER_CRATE; B->point_count = SCENE_PER_CRATE;
        for (int i = 0, k = b * SCENE_PER_CRATE; i < SCENE_NX; ++i)
            for (int j = 0; j < SCENE_NY; ++j)
                for (int l = 0; l < SCENE_NZ; ++l, ++k) {
                    hull[k].local[0] = (float)((i + 0.5) * (size[0] / SCENE_NX) - size[0] / 2);
                    hull[k].local[1] = (float)((j + 0.5) * (size[1] / SCENE_NY) - size[1] / 2);
                    hull[k].local[2] = (float)((l + 0.5) * (size[2] / SCENE_NZ) - size[2] / 2);
                    hull[k].volume = (float)(volume / SCENE_PER_CRATE);
                    hull[k].half_height = (float)(size[1] / SCENE_NY / 2);
                    hull[k].body = b;
                }
    }
}

/* the shape drawn at the crates' poses: the same box, corner 4 ix + 2 iy + iz, triangles 2 f and 2 f + 1 face f (-x +x -y +y -z +z),
 * every face counter-clockwise seen from outside */
static inline void scene_box(float corners[SCENE_BOX_VERTICES][3], int32_t idx[SCENE_BOX_TRIANGLES][3]) {
    static const int32_t quads[6][4] = {{0, 1, 3, 2}, {4, 6, 7, 5}, {0, 4, 5, 1}, {2, 3, 7, 6}, {0, 2, 6, 4}, {1, 5, 7, 3}};
    const double size[3] = SCENE_CRATE_SIZE;
    for (int v = 0; v < SCENE_BOX_VERTICES; ++v) {
        corners[v][0] = (float)((v & 4 ? 0.5 : -0.5) * size[0]);
        corners[v][1] = (float)((v & 2 ? 0.5 : -0.5) * size[1]);
        corners[v][2] = (float)((v & 1 ? 0.5 : -0.5) * size[2]);
    }
    for (int q = 0; q < 6; ++q) {
        idx[2 * q][0] = quads[q][0]; idx[2 * q][1] = quads[q][1]; idx[2 * q][2] = quads[q][2];
        idx[2 * q + 1][0] = quads[q][0]; idx[2 * q + 1][1] = quads[q][2]; idx[2 * q + 1][2] = quads[q][3];
    }
}

/* the grid: (cells + 1)^2 vertices around the node's origin, xyz[3 (cells + 1)^2] ... */
static inline void scene_grid_vertices(int cells, float cell, float *xyz) {
    for (int r = 0; r <= cells; ++r)
        for (int c = 0; c <= cells; ++c) {
            float *v = xyz + 3 * ((size_t)r * (size_t)(cells + 1) + (size_t)c);
            v[0] = (float)c * cell - 0.5f * cells * cell; v[1] = 0.0f; v[2] = (float)r * cell - 0.5f * cells * cell;
        }
}

/* ... and two triangles a cell, counter-clockwise seen from above, idx[6 cells^2] */
static inline void scene_grid_triangles(int cells, int32_t *idx) {
    for (int r = 0; r < cells; ++r)
        for (int c = 0; c < cells; ++c) {
            const int32_t a = r * (cells + 1) + c, b = a + 1, d = a + cells + 1, e = d + 1;
            int32_t *t = idx + 6 * ((size_t)r * (size_t)cells + (size_t)c);
            t[0] = a; t[1] = d; t[2] = b; t[3] = b; t[4] = d; t[5] = e;
        }
}

/* the grid as an ow_mesh; 0, or 1 after saying why on stderr.  The host's copies are freed on every path. */
static inline int scene_grid_create(ow_context *ctx, int cells, float cell, ow_mesh **mesh) {
    const int32_t num_vertices = (cells + 1) * (cells + 1), num_triangles = 2 * cells * cells;
    float *xyz = (float *)malloc((size_t)num_vertices * 3 * sizeof(float));
    int32_t *idx = (int32_t *)malloc((size_t)num_triangles * 3 * sizeof(int32_t));
    int failed = 1;
    if (!xyz || !idx) {
        fprintf(stderr, "out of memory\n");
    } else {
        scene_grid_vertices(cells, cell, xyz);
        scene_grid_triangles(cells, idx);
        failed = ow_mesh_create(ctx, xyz, num_vertices, idx, num_triangles, mesh) != OW_OK;
        if (failed) fprintf(stderr, "ocean_waves: %s\n", ow_last_error());
    }
    free(xyz); free(idx);
    return failed;
}

/* the panorama that stands in for main.tscn's PanoramaSkyMaterial, p[SCENE_PANO_W * SCENE_PANO_H * 4]: a zenith-to-horizon gradient above,
 * a darker one below, brighter towards the seam (+Z); integers only */
static inline void scene_panorama(unsigned char *p) {
    const int half = SCENE_PANO_H / 2;
    for (int j = 0; j < SCENE_PANO_H; ++j)
        for (int i = 0; i < SCENE_PANO_W; ++i) {
            unsigned char *t = p + 4 * (j * SCENE_PANO_W + i);
            const int up = j < half, k = up ? j : SCENE_PANO_H - 1 - j;   /* 0 at a pole .. half - 1 at the horizon */
            const int az = (20 * abs(2 * i - SCENE_PANO_W)) / SCENE_PANO_W;
            t[0] = (unsigned char)((up ? 60 + (150 * k) / (half - 1) : 30 + (40 * k) / (half - 1)) + az);
            t[1] = (unsigned char)((up ? 110 + (110 * k) / (half - 1) : 50 + (50 * k) / (half - 1)) + az);
            t[2] = (unsigned char)(up ? 200 + (40 * k) / (half - 1) : 70 + (60 * k) / (half - 1));
            t[3] = 255;
        }
}

/* the two spray textures, [SCENE_TEX * SCENE_TEX * 4] each, procedural because decoding the reference's sea_spray.png and generating its
 * NoiseTexture2D stay with the host.  albedo: white, alpha a puff that is 1 at the centre and 0 at the rim; dissolve: a value noise of
 * period SCENE_TEX in the red channel */
static inline void scene_textures(unsigned char *albedo, unsigned char *dissolve) {
    uint32_t lattice[8][8], s = 12345u;
    for (int j = 0; j < 8; ++j)
        for (int i = 0; i < 8; ++i) lattice[j][i] = ((s = s * 1664525u + 1013904223u) >> 24) & 0xffu;
    for (int j = 0; j < SCENE_TEX; ++j)
        for (int i = 0; i < SCENE_TEX; ++i) {
            unsigned char *a = albedo + 4 * (j * SCENE_TEX + i), *d = dissolve + 4 * (j * SCENE_TEX + i);
            const int dx = 2 * i + 1 - SCENE_TEX, dy = 2 * j + 1 - SCENE_TEX;     /* twice the distance from the centre, in texels */
            const int r2 = dx * dx + dy * dy, rim = SCENE_TEX * SCENE_TEX;
            a[0] = a[1] = a[2] = 255;
            a[3] = (unsigned char)(r2 >= rim ? 0 : 255 - (255 * r2) / rim);
            const int cx = i / 8, cy = j / 8, fx = i % 8, fy = j % 8;             /* bilinear over an 8 x 8 lattice, integers only */
            const uint32_t v00 = lattice[cy][cx], v10 = lattice[cy][(cx + 1) % 8], v01 = lattice[(cy + 1) % 8][cx], v11 = lattice[(cy + 1) % 8][(cx + 1) % 8];
            const uint32_t top = v00 * (uint32_t)(8 - fx) + v10 * (uint32_t)fx, bot = v01 * (uint32_t)(8 - fx) + v11 * (uint32_t)fx;
            d[0] = (unsigned char)((top * (uint32_t)(8 - fy) + bot * (uint32_t)fy) / 128u);   /* 0 .. 127: most particles clear it */
            d[1] = d[2] = d[0];
            d[3] = 255;
        }
}

/* the reference camera, main.tscn:119-120: at (0, 10, -25), looking towards +z, ten degrees down; Camera3D's default fov 75 and far 4000 */
static inline void scene_camera(ow_camera *cam, int width, int height) {
    static const float basis[9] = {-0.996195f, -0.0151344f, 0.0858316f, 0.0f, 0.984807f, 0.173648f, -0.0871557f, 0.172987f, -0.981061f};
    memset(cam, 0, sizeof *cam);
    memcpy(cam->basis, basis, sizeof basis);
    cam->position[0] = 0.0f; cam->position[1] = 10.0f; cam->position[2] = -25.0f;
    cam->fov_y_degrees = 75.0f;
    cam->max_distance = 4000.0f;
    cam->width = width; cam->height = height;
}

/* where main.gd:34-37 puts the clip map under a camera: ceil(camera.xz / cell) * cell */
static inline void scene_clipmap_origin(const ow_camera *cam, float cell, float origin[3]) {
    origin[0] = ceilf(cam->position[0] / cell) * cell; origin[1] = 0.0f; origin[2] = ceilf(cam->position[2] / cell) * cell;
}

/* the water mesh as Godot draws the material: the shader's distance falloff around the camera (water.gdshader:29, CAMERA_POSITION_WORLD.xz),
 * back faces culled */
static inline void scene_mesh_options(ow_mesh_options *opts, const ow_camera *cam) {
    ow_mesh_options_default(opts);
    opts->query_flags = OW_QUERY_DISTANCE_FALLOFF;
    opts->falloff_center_xz[0] = cam->position[0];
    opts->falloff_center_xz[1] = cam->position[2];
    opts->flags = OW_MESH_CULL_BACK;
}

/* a picture of width x height pixels resolved from records drawn at `down` times that: 0, or 1 after saying so on stderr */
static inline int scene_bad_size(int width, int height, int down) {
    const int bad = down < 1 || down > OW_PRESENT_MAX_DOWNSAMPLE || width < 1 || height < 1 || width > OW_RENDER_MAX_SIDE / down ||
                    height > OW_RENDER_MAX_SIDE / down;
    if (bad) fprintf(stderr, "bad image size\n");
    return bad;
}

/* count bytes to path: 0, or 1 after saying so on stderr */
static inline int scene_write_file(const char *path, const void *bytes, size_t count) {
    FILE *f = fopen(path, "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", path); return 1; }
    fwrite(bytes, 1, count, f);
    fclose(f);
    return 0;
}

/* the R, G, B of RGBA8 words as a binary PPM: 0, or 1 after saying so on stderr */
static inline int scene_write_ppm(const char *path, const unsigned char *rgba, int width, int height) {
    FILE *f = fopen(path, "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", path); return 1; }
    fprintf(f, "P6\n%d %d\n255\n", width, height);
    for (size_t i = 0; i < (size_t)width * (size_t)height; ++i) fwrite(rgba + 4 * i, 1, 3, f);
    fclose(f);
    return 0;
}

#endif

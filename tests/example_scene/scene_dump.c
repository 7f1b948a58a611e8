/* scene_dump.c -- the generators of examples/scene.h that only fill arrays, run on their own and written out raw, for
 * tests/test_example_scene.py to hold tests/scenes.py to: the crates' states and hull points, the box, the clip-map grid, the panorama
 * and the two spray textures.  Links nothing of the library; built with the sanitizers.
 *   scene_dump OUT_DIR */
#include "../../examples/scene.h"

static int dump(const char *dir, const char *name, const void *bytes, size_t count) {
    char path[1024];
    snprintf(path, sizeof path, "%s/%s.bin", dir, name);
    return scene_write_file(path, bytes, count);
}

int main(int argc, char **argv) {
    const char *dir = argc > 1 ? argv[1] : ".";
    const size_t num_vertices = (size_t)(SCENE_CELLS + 1) * (SCENE_CELLS + 1), num_triangles = (size_t)2 * SCENE_CELLS * SCENE_CELLS;
    const size_t pano = (size_t)SCENE_PANO_W * SCENE_PANO_H * 4, tex = (size_t)SCENE_TEX * SCENE_TEX * 4;
    ow_rigid_body *bodies = (ow_rigid_body *)malloc(SCENE_CRATES * sizeof *bodies);
    ow_hull_point *hull = (ow_hull_point *)malloc(SCENE_CRATES * SCENE_PER_CRATE * sizeof *hull);
    float corners[SCENE_BOX_VERTICES][3], *xyz = (float *)malloc(num_vertices * 3 * sizeof(float));
    int32_t idx[SCENE_BOX_TRIANGLES][3], *tri = (int32_t *)malloc(num_triangles * 3 * sizeof(int32_t));
    unsigned char *panorama = (unsigned char *)malloc(pano), *albedo = (unsigned char *)malloc(tex), *dissolve = (unsigned char *)malloc(tex);
    int failed = 1;
    if (bodies && hull && xyz && tri && panorama && albedo && dissolve) {
        scene_crates(bodies, hull);
        scene_box(corners, idx);
        scene_grid_vertices(SCENE_CELLS, SCENE_CELL, xyz);
        scene_grid_triangles(SCENE_CELLS, tri);
        scene_panorama(panorama);
        scene_textures(albedo, dissolve);
        failed = dump(dir, "crate_states", bodies, SCENE_CRATES * sizeof *bodies) || dump(dir, "crate_hull", hull, SCENE_CRATES * SCENE_PER_CRATE * sizeof *hull) ||
                 dump(dir, "box_vertices", corners, sizeof corners) || dump(dir, "box_triangles", idx, sizeof idx) ||
                 dump(dir, "grid_vertices", xyz, num_vertices * 3 * sizeof(float)) || dump(dir, "grid_triangles", tri, num_triangles * 3 * sizeof(int32_t)) ||
                 dump(dir, "panorama", panorama, pano) || dump(dir, "albedo", albedo, tex) || dump(dir, "dissolve", dissolve, tex);
    }
    free(bodies); free(hull); free(xyz); free(tri); free(panorama); free(albedo); free(dissolve);
    if (!failed) printf("cells=%d cell=%g crates=%d per_crate=%d panorama=%dx%d textures=%dx%d\n", SCENE_CELLS, (double)SCENE_CELL, SCENE_CRATES,
                        SCENE_PER_CRATE, SCENE_PANO_W, SCENE_PANO_H, SCENE_TEX, SCENE_TEX);
    return failed;
}

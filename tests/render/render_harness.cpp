// render_harness.cpp -- godotoceanwaves_amd/csrc/ow_render.h and ow_shading.h compiled as plain C++ (g++ -ffp-contract=off): log_f32, the
// pixel rays and k_render_view's per-pixel body over maps in host memory, the pixels taken one after the other.
// Test infrastructure (tests/test_render_view.py); the GPU records and RGBA8 words are held to these bit for bit.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "ow_render.h"

extern "C" {

int harness_render_sizes(int *sizes) {
    sizes[0] = (int)sizeof(ow::RenderPixel);
    sizes[1] = (int)offsetof(ow::RenderPixel, status);
    sizes[2] = (int)offsetof(ow::RenderPixel, p);
    sizes[3] = (int)offsetof(ow::RenderPixel, dist);
    sizes[4] = (int)offsetof(ow::RenderPixel, normal);
    sizes[5] = (int)offsetof(ow::RenderPixel, color);
    sizes[6] = (int)sizeof(ow::ShadeParams);
    sizes[7] = (int)sizeof(ow::CameraParams);
    return 0;
}

void harness_log(const float *x, int count, float *out) {
    for (int i = 0; i < count; ++i) out[i] = ow::log_f32(x[i]);
}

// camera: position[3], basis[9], tan(fov / 2), aspect, max_distance as the runtime resolves them from ow_camera
static ow::CameraParams camera_of(const float *camera, int width, int height) {
    ow::CameraParams cam;
    memcpy(cam.o, camera, 3 * sizeof(float));
    memcpy(cam.B, camera + 3, 9 * sizeof(float));
    cam.tan_half_fov = camera[12];
    cam.aspect = camera[13];
    cam.max_distance = camera[14];
    cam.width = width;
    cam.height = height;
    return cam;
}

// the W x H pixel rays, row-major from the top-left pixel
void harness_pixel_rays(const float *camera, int width, int height, ow::Ray *out) {
    const ow::CameraParams cam = camera_of(camera, width, height);
    for (int j = 0; j < height; ++j)
        for (int i = 0; i < width; ++i) out[(size_t)j * width + i] = ow::pixel_ray(cam, i, j);
}

// shade: the 22 floats of ow::ShadeParams in order, as the runtime resolves them from ow_render_options; the ray cast's settings as
// harness_raycast takes them.  rgba and pixels may each be NULL.
void harness_render(const uint16_t *disp, const uint16_t *norm, int n, int cascades, const float *map_scales, const float *camera, int width,
                    int height, const float *shade, int max_iterations, float tolerance, int falloff, float cx, float cz, float water_level,
                    float spacing, float ray_tolerance, int max_samples, uint32_t *rgba, ow::RenderPixel *pixels) {
    static_assert(sizeof(ow::ShadeParams) == 22 * sizeof(float), "ShadeParams is 22 floats");
    ow::SurfaceScales sc;
    memset(&sc, 0, sizeof(sc));
    memcpy(sc.s, map_scales, (size_t)cascades * 4 * sizeof(float));
    ow::RaycastParams rp;
    rp.qp.max_iterations = max_iterations;
    rp.qp.tolerance = tolerance;
    rp.qp.falloff = falloff;
    rp.qp.center[0] = cx;
    rp.qp.center[1] = cz;
    rp.water_level = water_level;
    rp.spacing = spacing;
    rp.tolerance = ray_tolerance;
    rp.max_samples = max_samples;
    ow::ShadeParams sp;
    memcpy(&sp, shade, sizeof(sp));
    const ow::CameraParams cam = camera_of(camera, width, height);
    const ow::u16x4 *d = (const ow::u16x4 *)disp;
    uint32_t bound[8] = {0};
    for (int c = 0; c < cascades; ++c)
        for (size_t i = 0; i < (size_t)n * n; ++i) {
            const uint32_t m = ow::dy_magnitude_bits(d[(size_t)c * n * n + i]);
            if (m > bound[c]) bound[c] = m;
        }
    const float hw = ow::slab_half_height(bound, cascades, sc);
    for (int j = 0; j < height; ++j)
        for (int i = 0; i < width; ++i) {
            uint32_t word;
            const ow::RenderPixel px = ow::render_pixel(d, (const ow::u16x4 *)norm, n, cascades, sc, rp, cam, sp, hw, i, j, &word);
            const size_t at = (size_t)j * width + i;
            if (rgba) rgba[at] = word;
            if (pixels) pixels[at] = px;
        }
}

}  // extern "C"

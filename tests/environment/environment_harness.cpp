// environment_harness.cpp -- godotoceanwaves_amd/csrc/ow_environment.h compiled as plain C++ (g++ -ffp-contract=off): the CPU build of the
// environment pass and the present that tests/test_environment.py holds to an FP64 twin written from the definition
// (tests/environment_twin.py) and that the GPU kernels are held to bit for bit.  With -DENVIRONMENT_HARNESS_MAIN it is a stand-alone
// program that reads a case file (the two headers below, then the panorama and the records), applies the pass twice, presents and writes
// the results: the form the sanitizers run.
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "ow_environment.h"

using namespace ow;

extern "C" {

// one pass, every field four bytes: what the runtime resolves from its arguments
struct EnvCase {
    int32_t width, height;
    float cam[15];  // position, basis rows, tan(fov / 2), aspect, max_distance
    int32_t fog_mode;
    float density, depth_begin, depth_end, depth_curve, aerial_perspective, sun_scatter;
    float light_color[3], sun_color[3], sun_direction[3], sky_color[3];
    int32_t has_sky, sky_width, sky_height, sky_srgb;
    float energy;
};
// one present; width x height is the size of the records
struct PresentCase {
    int32_t width, height;
    int32_t downsample, tonemap;
    float exposure, white;
    int32_t srgb;
    float brightness, contrast, saturation;
};

constexpr int kEnvStages = 10;      // per record: ray[3], sky[3], amount, fog[3]
constexpr int kPresentStages = 12;  // per output pixel: exposed[3], mapped[3], encoded[3], adjusted[3]

// sizeof and the offsets the Python side mirrors
void harness_environment_sizes(int *out) {
    out[0] = (int)sizeof(SkyOptions);
    out[1] = (int)offsetof(SkyOptions, energy);
    out[2] = (int)sizeof(EnvironmentOptions);
    out[3] = (int)offsetof(EnvironmentOptions, flags);
    out[4] = (int)offsetof(EnvironmentOptions, light_color);
    out[5] = (int)offsetof(EnvironmentOptions, sun_direction);
    out[6] = (int)offsetof(EnvironmentOptions, reserved);
    out[7] = (int)sizeof(PresentOptions);
    out[8] = (int)offsetof(PresentOptions, srgb);
    out[9] = (int)offsetof(PresentOptions, reserved);
    out[10] = (int)sizeof(EnvCase);
    out[11] = (int)sizeof(PresentCase);
}

void harness_atan2(const float *y, const float *x, int n, float *out) {
    for (int i = 0; i < n; ++i) out[i] = atan2_f32(y[i], x[i]);
}
void harness_acos(const float *y, int n, float *out) {
    for (int i = 0; i < n; ++i) out[i] = acos_f32(y[i]);
}

}  // extern "C"

namespace {
CameraParams camera_of(const EnvCase &h) {
    CameraParams cam;
    memcpy(cam.o, h.cam, 3 * sizeof(float));
    memcpy(cam.B, h.cam + 3, 9 * sizeof(float));
    cam.tan_half_fov = h.cam[12];
    cam.aspect = h.cam[13];
    cam.max_distance = h.cam[14];
    cam.width = h.width;
    cam.height = h.height;
    return cam;
}
// as the runtime resolves ow_environment_options and the sky (ow_sky_host.hip resolve_environment_options, environment_apply)
EnvParams params_of(const EnvCase &h, const CameraParams &cam, const uint32_t *texels, const float *table) {
    EnvParams ep;
    memset(&ep, 0, sizeof(ep));
    const double lx = h.sun_direction[0], ly = h.sun_direction[1], lz = h.sun_direction[2];
    const double len = sqrt(lx * lx + ly * ly + lz * lz);
    ep.fog_mode = h.fog_mode;
    ep.density = h.density;
    ep.begin = h.depth_begin;
    ep.end = h.depth_end;
    ep.curve = h.depth_curve;
    ep.aerial = h.aerial_perspective;
    ep.scatter = h.sun_scatter;
    for (int k = 0; k < 3; ++k) {
        ep.light_color[k] = h.light_color[k];
        ep.sun_color[k] = h.sun_color[k];
        ep.sun[k] = len > 0.0 ? (float)((double)h.sun_direction[k] / len) : 0.0f;
        ep.sky_color[k] = h.sky_color[k];
    }
    ep.energy = 1.0f;
    if (h.has_sky) {
        ep.has_sky = 1;
        ep.sky = SprayTexture{texels, h.sky_width, h.sky_height, h.sky_srgb};
        ep.srgb = table;
        ep.energy = h.energy;
    }
    ep.camera_ok = mesh_camera_ok(cam) ? 1 : 0;
    return ep;
}
PresentParams present_of(const PresentCase &h) {
    PresentParams pp;
    pp.s = h.downsample == 0 ? 1 : h.downsample;
    pp.inv = 1.0f / (float)(pp.s * pp.s);
    pp.tonemap = h.tonemap;
    pp.exposure = h.exposure;
    pp.white = h.white;
    pp.srgb = h.srgb;
    pp.brightness = h.brightness;
    pp.contrast = h.contrast;
    pp.saturation = h.saturation;
    return pp;
}
}  // namespace

extern "C" {

// the panorama along n unit directions, times the energy (the case's camera and fog are not read)
void harness_sky_lookup(const EnvCase *hp, const uint32_t *texels, const float *dirs, int n, float *out) {
    float table[256];
    spray_srgb_table(table);
    const SprayTexture t{texels, hp->sky_width, hp->sky_height, hp->sky_srgb};
    for (int i = 0; i < n; ++i) {
        sky_texture(t, table, dirs + 3 * (size_t)i, out + 3 * (size_t)i);
        for (int k = 0; k < 3; ++k) out[3 * (size_t)i + k] *= hp->energy;
    }
}

// the fog amount at n distances
void harness_fog_amount(const EnvCase *hp, const float *d, int n, float *out) {
    const CameraParams cam = camera_of(*hp);
    const EnvParams ep = params_of(*hp, cam, nullptr, nullptr);
    for (int i = 0; i < n; ++i) out[i] = fog_amount(ep, d[i]);
}

// The pass: k_environment_apply's route over width x height records in place.  stages: kEnvStages floats per record, or null.
void harness_environment_apply(const EnvCase *hp, const uint32_t *texels, void *pixels_inout, float *stages) {
    const EnvCase &h = *hp;
    const CameraParams cam = camera_of(h);
    float table[256];
    spray_srgb_table(table);
    const EnvParams ep = params_of(h, cam, texels, table);
    RenderPixel *pixels = (RenderPixel *)pixels_inout;
    if (stages) memset(stages, 0, (size_t)h.width * h.height * kEnvStages * sizeof(float));
    if (!ep.camera_ok) return;  // launch_environment_apply launches nothing
    for (int j = 0; j < h.height; ++j)
        for (int i = 0; i < h.width; ++i) {
            const size_t at = (size_t)j * h.width + i;
            const EnvPixel px = environment_pixel(ep, cam, i, j, pixels[at].t, pixels[at].status, pixels[at].color);
            if (stages) {
                float *s = stages + at * kEnvStages;
                for (int k = 0; k < 3; ++k) {
                    s[k] = px.ray[k];
                    s[3 + k] = px.sky[k];
                    s[7 + k] = px.fog[k];
                }
                s[6] = px.amount;
            }
            if (!px.changed) continue;
            for (int k = 0; k < 3; ++k) pixels[at].color[k] = px.color[k];
            pixels[at].status = px.status;
        }
}

// The present: k_present's route.  rgba_out: (width / s) x (height / s) words or null; linear_out: as many float4 or null; stages:
// kPresentStages floats per output pixel, or null.
void harness_present(const PresentCase *hp, const void *pixels_in, uint32_t *rgba_out, float *linear_out, float *stages) {
    const PresentParams pp = present_of(*hp);
    const RenderPixel *pixels = (const RenderPixel *)pixels_in;
    const int ow_ = hp->width / pp.s, oh = hp->height / pp.s;
    const size_t row_stride = (size_t)ow_ * pp.s;
    for (int oy = 0; oy < oh; ++oy)
        for (int ox = 0; ox < ow_; ++ox) {
            const size_t at = (size_t)oy * ow_ + ox;
            float lin[4];
            PresentStages st;
            const uint32_t word = present_pixel(pp, pixels + (size_t)oy * pp.s * row_stride + (size_t)ox * pp.s, row_stride, lin, st);
            if (rgba_out) rgba_out[at] = word;
            if (linear_out) memcpy(linear_out + 4 * at, lin, sizeof(lin));
            if (stages) {
                float *s = stages + at * kPresentStages;
                memcpy(s, st.exposed, 12);
                memcpy(s + 3, st.mapped, 12);
                memcpy(s + 6, st.encoded, 12);
                memcpy(s + 9, st.adjusted, 12);
            }
        }
}

}  // extern "C"

#ifdef ENVIRONMENT_HARNESS_MAIN
namespace {
bool read_all(FILE *f, void *dst, size_t bytes) { return bytes == 0 || (dst && fread(dst, 1, bytes, f) == bytes); }
bool finite(float v) { return fabsf(v) <= 3.4028235e38f; }
}  // namespace

// environment_harness_main CASE OUT: reads the two headers and the arrays (panorama texels, records), applies the pass twice, presents, and
// writes the records after the first pass, the RGBA8 words and the linear pixels
int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s CASE OUT\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    EnvCase h;
    PresentCase p;
    if (!read_all(f, &h, sizeof(h)) || !read_all(f, &p, sizeof(p)) || h.width < 1 || h.height < 1 || h.width > 8192 || h.height > 8192 ||
        p.width != h.width || p.height != h.height || p.downsample < 0 || p.downsample > kPresentMaxDownsample ||
        h.width % (p.downsample ? p.downsample : 1) != 0 || h.height % (p.downsample ? p.downsample : 1) != 0 ||
        (h.has_sky && (h.sky_width < 1 || h.sky_height < 1 || h.sky_width > kSkyMaxSide || h.sky_height > kSkyMaxSide))) {
        fprintf(stderr, "bad case header\n");
        return 2;
    }
    const int s = p.downsample ? p.downsample : 1;
    const size_t count = (size_t)h.width * h.height, out_count = (size_t)(h.width / s) * (h.height / s);
    std::vector<uint32_t> texels(h.has_sky ? (size_t)h.sky_width * h.sky_height : 0), rgba(out_count);
    std::vector<RenderPixel> pixels(count);
    std::vector<float> linear(4 * out_count);
    if (!read_all(f, texels.data(), texels.size() * 4) || !read_all(f, pixels.data(), pixels.size() * sizeof(RenderPixel))) {
        fprintf(stderr, "short case file\n");
        return 2;
    }
    fclose(f);
    harness_environment_apply(&h, texels.data(), pixels.data(), nullptr);
    const std::vector<RenderPixel> once = pixels;
    harness_environment_apply(&h, texels.data(), pixels.data(), nullptr);
    const bool idempotent = memcmp(once.data(), pixels.data(), count * sizeof(RenderPixel)) == 0;
    harness_present(&p, pixels.data(), rgba.data(), linear.data(), nullptr);
    int bad = 0, marked = 0;
    for (const float v : linear) bad += !finite(v);
    for (const RenderPixel &px : pixels) marked += (px.status & kRayEnvironment) ? 1 : 0;
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(once.data(), sizeof(RenderPixel), once.size(), o);
    fwrite(rgba.data(), 4, rgba.size(), o);
    fwrite(linear.data(), 4, linear.size(), o);
    fclose(o);
    printf("marked=%d idempotent=%d not_finite=%d\n", marked, idempotent ? 1 : 0, bad);
    printf("ok\n");
    return (bad || !idempotent) ? 1 : 0;
}
#endif

// sky_light_harness.cpp -- godotoceanwaves_amd/csrc/ow_sky_light.h compiled as plain C++ (g++ -ffp-contract=off): the CPU build of the
// radiance pyramid and of the sky-light pass that tests/test_sky_light.py holds to an FP64 twin written from the definition
// (tests/sky_light_twin.py) and that the GPU kernels are held to bit for bit.  It exposes the stages: the tables, M_k, R_k, E, and per
// record V, R, lod, radiance, env, irradiance, ambient and spec.  With -DSKY_LIGHT_HARNESS_MAIN it is a stand-alone program that reads a
// case file (the two headers below, then the panorama and the records), builds the pyramid, applies the pass twice and writes the results:
// the form the sanitizers run.
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "ow_sky_light.h"

using namespace ow;

extern "C" {

// a pyramid, every field four bytes: the sky and the options with their zeros resolved
struct RadianceCase {
    int32_t sky_width, sky_height, sky_srgb;
    float energy;
    int32_t levels, samples, base_width;
};
// one pass
struct LightCase {
    int32_t width, height;
    float cam[15];  // position, basis rows, tan(fov / 2), aspect, max_distance
    float ambient_energy, reflection_energy, specular;
};

constexpr int kLightStages = 21;  // per record: view[3], reflect[3], lod, radiance[3], env[2], irradiance[3], ambient[3], spec[3]

// sizeof and the offsets the Python side mirrors
void harness_sky_light_sizes(int *out) {
    out[0] = (int)sizeof(RadianceOptions);
    out[1] = (int)offsetof(RadianceOptions, reserved);
    out[2] = (int)sizeof(SkyLightOptions);
    out[3] = (int)offsetof(SkyLightOptions, flags);
    out[4] = (int)offsetof(SkyLightOptions, reserved);
    out[5] = (int)sizeof(RadianceCase);
    out[6] = (int)sizeof(LightCase);
    out[7] = kLightStages;
    out[8] = kRaySkyLit;
}

// the level sizes: returns 0 where the pyramid is refused; out: pre, chain, source, then chain (width, height) pairs
int harness_radiance_plan(int sky_width, int sky_height, int levels, int base_width, int *out) {
    RadiancePlan p;
    if (!radiance_plan(sky_width, sky_height, levels, base_width, &p)) return 0;
    out[0] = p.pre;
    out[1] = p.chain;
    out[2] = p.source;
    for (int k = 0; k < p.chain; ++k) {
        out[3 + 2 * k] = p.width[k];
        out[4 + 2 * k] = p.height[k];
    }
    return 1;
}
void harness_radiance_dir_table(int n, int rows, float *out) { radiance_dir_table(n, rows != 0, out); }
void harness_radiance_sample_table(double r, int S, float *out) { radiance_sample_table(r, S, out); }

}  // extern "C"

namespace {
struct Texture {
    int width = 0, height = 0;
    std::vector<float> texels;
    RadianceLevel level() const { return RadianceLevel{texels.data(), width, height}; }
};
// the CPU build of a pyramid: launch_radiance_build's route, texel by texel in each kernel's order
struct Pyramid {
    RadiancePlan plan{};
    std::vector<Texture> M, R;
    Texture E;
    std::vector<std::vector<float>> col, row, samples;
};

Texture box(const Texture &in) {
    Texture out;
    out.width = in.width / 2;
    out.height = in.height / 2;
    out.texels.resize((size_t)out.width * out.height * 4);
    for (int j = 0; j < out.height; ++j)
        for (int i = 0; i < out.width; ++i) radiance_box_texel(in.texels.data(), in.width, i, j, &out.texels[4 * ((size_t)j * out.width + i)]);
    return out;
}

Pyramid *build(const RadianceCase &h, const uint32_t *texels) {
    Pyramid *P = new Pyramid();
    if (!radiance_plan(h.sky_width, h.sky_height, h.levels, h.base_width, &P->plan)) {
        delete P;
        return nullptr;
    }
    RadiancePlan &p = P->plan;
    p.samples = h.samples;
    float table[256];
    spray_srgb_table(table);
    const SprayTexture sky{texels, h.sky_width, h.sky_height, h.sky_srgb};
    Texture t;
    t.width = h.sky_width;
    t.height = h.sky_height;
    t.texels.resize((size_t)t.width * t.height * 4);
    for (int j = 0; j < t.height; ++j)
        for (int i = 0; i < t.width; ++i) radiance_decode_texel(sky, table, h.energy, i, j, &t.texels[4 * ((size_t)j * t.width + i)]);
    for (int i = 0; i < p.pre; ++i) t = box(t);
    P->M.push_back(t);
    for (int k = 1; k < p.chain; ++k) P->M.push_back(box(P->M[k - 1]));
    P->col.resize(p.chain);
    P->row.resize(p.chain);
    for (int k = 0; k < p.chain; ++k) {
        P->col[k].resize(2 * (size_t)p.width[k]);
        P->row[k].resize(2 * (size_t)p.height[k]);
        radiance_dir_table(p.width[k], false, P->col[k].data());
        radiance_dir_table(p.height[k], true, P->row[k].data());
    }
    P->samples.resize(p.levels);
    P->R.resize(p.levels);
    P->R[0] = P->M[0];
    for (int k = 1; k < p.levels; ++k) {
        P->samples[k].resize(4 * (size_t)h.samples);
        radiance_sample_table((double)k / (double)(p.levels - 1), h.samples, P->samples[k].data());
        Texture &r = P->R[k];
        r.width = p.width[k];
        r.height = p.height[k];
        r.texels.resize((size_t)r.width * r.height * 4);
        const RadianceLevel m = P->M[k].level();
        for (int j = 0; j < r.height; ++j)
            for (int i = 0; i < r.width; ++i)
                radiance_prefilter_texel(m, P->col[k].data(), P->row[k].data(), P->samples[k].data(), h.samples, i, j, &r.texels[4 * ((size_t)j * r.width + i)]);
    }
    std::vector<float> ecol(2 * kIrradianceWidth), erow(2 * kIrradianceHeight);
    radiance_dir_table(kIrradianceWidth, false, ecol.data());
    radiance_dir_table(kIrradianceHeight, true, erow.data());
    P->E.width = kIrradianceWidth;
    P->E.height = kIrradianceHeight;
    P->E.texels.resize((size_t)kIrradianceWidth * kIrradianceHeight * 4);
    const RadianceLevel src = P->M[p.source].level();
    for (int j = 0; j < kIrradianceHeight; ++j)
        for (int i = 0; i < kIrradianceWidth; ++i)
            radiance_irradiance_texel(src, P->col[p.source].data(), P->row[p.source].data(), ecol.data(), erow.data(), i, j,
                                      &P->E.texels[4 * ((size_t)j * kIrradianceWidth + i)]);
    return P;
}

CameraParams camera_of(const LightCase &h) {
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
// as the runtime resolves ow_radiance_light_options and the pyramid (ow_sky_host.hip resolve_radiance_light_options, radiance_light_apply)
SkyLightParams params_of(const LightCase &h, const CameraParams &cam, const Pyramid &P) {
    SkyLightParams lp;
    memset(&lp, 0, sizeof(lp));
    lp.levels = P.plan.levels;
    lp.ambient_energy = h.ambient_energy;
    lp.reflection_energy = h.reflection_energy;
    sky_light_fresnel(h.specular, lp.f0, lp.f50);
    for (int k = 0; k < P.plan.levels; ++k) lp.R[k] = P.R[k].level();
    lp.E = P.E.level();
    lp.camera_ok = mesh_camera_ok(cam) ? 1 : 0;
    return lp;
}
const Texture *texture_of(const Pyramid &P, int kind, int k) {
    if (kind == 0 && k >= 0 && k < (int)P.R.size()) return &P.R[k];
    if (kind == 1 && k >= 0 && k < (int)P.M.size()) return &P.M[k];
    if (kind == 2) return &P.E;
    return nullptr;
}
}  // namespace

extern "C" {

// a pyramid of a panorama; null where the sizes are refused
void *harness_radiance_new(const RadianceCase *h, const uint32_t *texels) { return build(*h, texels); }
void harness_radiance_free(void *p) { delete (Pyramid *)p; }
// kind 0: R_k, 1: M_k, 2: E.  size: width, height; out (may be null): the texels.  Returns 0 for a texture that does not exist.
int harness_radiance_get(const void *p, int kind, int k, int *size, float *out) {
    const Texture *t = texture_of(*(const Pyramid *)p, kind, k);
    if (!t) return 0;
    size[0] = t->width;
    size[1] = t->height;
    if (out) memcpy(out, t->texels.data(), t->texels.size() * sizeof(float));
    return 1;
}
// a texture along n directions
void harness_radiance_lookup(const void *p, int kind, int k, const float *dirs, int n, float *out) {
    const Texture *t = texture_of(*(const Pyramid *)p, kind, k);
    for (int i = 0; t && i < n; ++i) radiance_tap(t->level(), dirs + 3 * (size_t)i, out + 3 * (size_t)i);
}

// The pass: k_sky_light_apply's route over width x height records in place.  stages: kLightStages floats per record, or null.
void harness_sky_light_apply(const void *p, const LightCase *hp, void *pixels_inout, float *stages) {
    const LightCase &h = *hp;
    const CameraParams cam = camera_of(h);
    const SkyLightParams lp = params_of(h, cam, *(const Pyramid *)p);
    RenderPixel *pixels = (RenderPixel *)pixels_inout;
    if (stages) memset(stages, 0, (size_t)h.width * h.height * kLightStages * sizeof(float));
    if (!lp.camera_ok) return;  // launch_sky_light_apply launches nothing
    for (int j = 0; j < h.height; ++j)
        for (int i = 0; i < h.width; ++i) {
            const size_t at = (size_t)j * h.width + i;
            RenderPixel &r = pixels[at];
            const SkyLightPixel px = sky_light_pixel(lp, cam, i, j, r.status, r.position, r.albedo, r.normal, r.roughness, r.color);
            if (stages) {
                float *s = stages + at * kLightStages;
                memcpy(s, px.view, 12);
                memcpy(s + 3, px.reflect, 12);
                s[6] = px.lod;
                memcpy(s + 7, px.radiance, 12);
                memcpy(s + 10, px.env, 8);
                memcpy(s + 12, px.irradiance, 12);
                memcpy(s + 15, px.ambient, 12);
                memcpy(s + 18, px.spec, 12);
            }
            if (!px.changed) continue;
            for (int k = 0; k < 3; ++k) r.color[k] = px.color[k];
            r.status = px.status;
        }
}

}  // extern "C"

#ifdef SKY_LIGHT_HARNESS_MAIN
namespace {
bool read_all(FILE *f, void *dst, size_t bytes) { return bytes == 0 || (dst && fread(dst, 1, bytes, f) == bytes); }
bool finite(float v) { return fabsf(v) <= 3.4028235e38f; }
}  // namespace

// sky_light_harness_main CASE OUT: reads the two headers and the arrays (panorama texels, records), builds the pyramid, applies the pass
// twice, and writes every level, E and the records after the first pass
int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s CASE OUT\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    RadianceCase rc;
    LightCase lc;
    if (!read_all(f, &rc, sizeof(rc)) || !read_all(f, &lc, sizeof(lc)) || rc.sky_width < 1 || rc.sky_height < 1 || rc.sky_width > kSkyMaxSide ||
        rc.sky_height > kSkyMaxSide || rc.levels < 2 || rc.levels > kRadianceMaxLevels || rc.samples < 1 || rc.samples > kRadianceMaxSamples ||
        rc.base_width < kRadianceMinBase || rc.base_width > kRadianceMaxBase || lc.width < 1 || lc.height < 1 || lc.width > 8192 || lc.height > 8192) {
        fprintf(stderr, "bad case header\n");
        return 2;
    }
    std::vector<uint32_t> texels((size_t)rc.sky_width * rc.sky_height);
    std::vector<RenderPixel> pixels((size_t)lc.width * lc.height);
    if (!read_all(f, texels.data(), texels.size() * 4) || !read_all(f, pixels.data(), pixels.size() * sizeof(RenderPixel))) {
        fprintf(stderr, "short case file\n");
        return 2;
    }
    fclose(f);
    Pyramid *P = build(rc, texels.data());
    if (!P) {
        fprintf(stderr, "the sizes are refused\n");
        return 2;
    }
    harness_sky_light_apply(P, &lc, pixels.data(), nullptr);
    const std::vector<RenderPixel> once = pixels;
    harness_sky_light_apply(P, &lc, pixels.data(), nullptr);
    const bool idempotent = memcmp(once.data(), pixels.data(), pixels.size() * sizeof(RenderPixel)) == 0;
    int bad = 0, marked = 0;
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    for (const Texture &t : P->R) {
        for (const float v : t.texels) bad += !finite(v);
        fwrite(t.texels.data(), 4, t.texels.size(), o);
    }
    for (const float v : P->E.texels) bad += !finite(v);
    fwrite(P->E.texels.data(), 4, P->E.texels.size(), o);
    for (const RenderPixel &px : once) {
        marked += (px.status & kRaySkyLit) ? 1 : 0;
        for (int k = 0; k < 3; ++k) bad += !finite(px.color[k]) ? 1 : 0;
    }
    fwrite(once.data(), sizeof(RenderPixel), once.size(), o);
    fclose(o);
    delete P;
    printf("marked=%d idempotent=%d not_finite=%d\n", marked, idempotent ? 1 : 0, bad);
    printf("ok\n");
    return !idempotent ? 1 : 0;
}
#endif

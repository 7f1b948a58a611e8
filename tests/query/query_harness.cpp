// query_harness.cpp -- godotoceanwaves_amd/csrc/ow_surface.h compiled as plain C++ (g++ -ffp-contract=off): the per-point code of
// k_sample_surface and k_query_surface, run over maps in host memory.  Test infrastructure (tests/test_surface_query.py); the GPU
// records are held to these bit for bit.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "ow_surface.h"

namespace {
ow::SurfaceScales scales_of(const float *map_scales, int cascades) {
    ow::SurfaceScales sc;
    memset(&sc, 0, sizeof(sc));
    memcpy(sc.s, map_scales, (size_t)cascades * 4 * sizeof(float));
    return sc;
}
}  // namespace

extern "C" {

int harness_record_sizes(int *sample_bytes, int *query_bytes, int *sample_offset) {
    *sample_bytes = (int)sizeof(ow::SurfaceSample);
    *query_bytes = (int)sizeof(ow::SurfaceQuery);
    *sample_offset = (int)offsetof(ow::SurfaceQuery, sample);
    return 0;
}

// disp / norm: [cascades][n][n][4] FP16 bits; map_scales: 4 floats per cascade; xz: count (x, z) pairs
void harness_sample(const uint16_t *disp, const uint16_t *norm, int n, int cascades, const float *map_scales, const float *xz, int count,
                    ow::SurfaceSample *out) {
    const ow::SurfaceScales sc = scales_of(map_scales, cascades);
    for (int i = 0; i < count; ++i)
        out[i] = ow::sample_point((const ow::u16x4 *)disp, (const ow::u16x4 *)norm, n, cascades, sc, xz[2 * i], xz[2 * i + 1]);
}

// the solver's settings as the runtime resolves them from ow_query_options
void harness_query(const uint16_t *disp, const uint16_t *norm, int n, int cascades, const float *map_scales, const float *xz, int count,
                   int max_iterations, float tolerance, int falloff, float cx, float cz, ow::SurfaceQuery *out) {
    const ow::SurfaceScales sc = scales_of(map_scales, cascades);
    ow::QueryParams qp;
    qp.max_iterations = max_iterations;
    qp.tolerance = tolerance;
    qp.falloff = falloff;
    qp.center[0] = cx;
    qp.center[1] = cz;
    for (int i = 0; i < count; ++i)
        out[i] = ow::query_point((const ow::u16x4 *)disp, (const ow::u16x4 *)norm, n, cascades, sc, qp, xz[2 * i], xz[2 * i + 1]);
}

void harness_exp(const float *a, int count, float *out) {
    for (int i = 0; i < count; ++i) out[i] = ow::exp_f32(a[i]);
}

}  // extern "C"

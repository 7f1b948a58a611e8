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

// query_eval at count (p, q) pairs, pq = (px, pz, qx, qz) each: out = (F[2], J[2][2] row-major, f, r), eight floats per pair
void harness_eval(const uint16_t *disp, int n, int cascades, const float *map_scales, const float *pq, int count, int falloff, float cx,
                  float cz, float *out) {
    const ow::SurfaceScales sc = scales_of(map_scales, cascades);
    ow::QueryParams qp;
    qp.max_iterations = ow::kQueryDefaultIterations;
    qp.tolerance = ow::kQueryDefaultTolerance;
    qp.falloff = falloff;
    qp.center[0] = cx;
    qp.center[1] = cz;
    for (int i = 0; i < count; ++i) {
        const float *a = pq + 4 * i;
        const ow::QueryEval e = ow::query_eval((const ow::u16x4 *)disp, n, cascades, sc, qp, a[0], a[1], a[2], a[3]);
        const float rec[8] = {e.F[0], e.F[1], e.J[0][0], e.J[0][1], e.J[1][0], e.J[1][1], e.f, e.r};
        memcpy(out + 8 * i, rec, sizeof(rec));
    }
}

// make_tap's integers and weights at count normalised (u, v) pairs: taps = (r0, r1, c0, c1) each, weights = (wx, wy) each
void harness_tap(const float *uv, int count, int n, int32_t *taps, float *weights) {
    for (int i = 0; i < count; ++i) {
        const ow::Tap t = ow::make_tap(uv[2 * i], uv[2 * i + 1], n);
        const int32_t v[4] = {t.r0, t.r1, t.c0, t.c1};
        memcpy(taps + 4 * i, v, sizeof(v));
        weights[2 * i] = t.wx;
        weights[2 * i + 1] = t.wy;
    }
}

void harness_exp(const float *a, int count, float *out) {
    for (int i = 0; i < count; ++i) out[i] = ow::exp_f32(a[i]);
}

}  // extern "C"

// velocity_harness.cpp -- godotoceanwaves_amd/csrc/ow_velocity.h compiled as plain C++ (g++ -ffp-contract=off): the per-point body of
// k_query_velocity and the flagged per-point evaluation of k_buoyancy_points_moving with the per-body sum of k_buoyancy_bodies, over layers
// in host memory.  Test infrastructure (tests/test_water_velocity.py); the GPU records are held to these bit for bit.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "ow_velocity.h"

extern "C" {

int harness_velocity_sizes(int *sizes) {
    sizes[0] = (int)sizeof(ow::SurfaceVelocity);
    sizes[1] = (int)offsetof(ow::SurfaceVelocity, height);
    sizes[2] = (int)offsetof(ow::SurfaceVelocity, p);
    sizes[3] = (int)offsetof(ow::SurfaceVelocity, converged);
    return 0;
}

static ow::SurfaceScales scales_of(const float *map_scales, int cascades) {
    ow::SurfaceScales sc;
    memset(&sc, 0, sizeof(sc));
    memcpy(sc.s, map_scales, (size_t)cascades * 4 * sizeof(float));
    return sc;
}
static ow::QueryParams query_params(int max_iterations, float tolerance, int falloff, float cx, float cz) {
    ow::QueryParams qp;
    qp.max_iterations = max_iterations;
    qp.tolerance = tolerance;
    qp.falloff = falloff;
    qp.center[0] = cx;
    qp.center[1] = cz;
    return qp;
}

void harness_query_velocity(const uint16_t *disp, const uint16_t *vel, int n, int cascades, const float *map_scales, const float *xz, int count,
                            int max_iterations, float tolerance, int falloff, float cx, float cz, ow::SurfaceVelocity *out) {
    const ow::SurfaceScales sc = scales_of(map_scales, cascades);
    const ow::QueryParams qp = query_params(max_iterations, tolerance, falloff, cx, cz);
    for (int i = 0; i < count; ++i)
        out[i] = ow::velocity_point((const ow::u16x4 *)disp, (const ow::u16x4 *)vel, n, cascades, sc, qp, xz[2 * i], xz[2 * i + 1]);
}

// ow_buoyancy with OW_BUOYANCY_WATER_VELOCITY (cold or warm start as the harness of tests/buoyancy/)
void harness_buoyancy_moving(const uint16_t *disp, const uint16_t *vel, int n, int cascades, const float *map_scales, const ow::BuoyancyBody *bodies,
                             int num_bodies, const ow::HullPoint *hull, int num_points, int max_iterations, float tolerance, int falloff, float cx,
                             float cz, float density, float rho_g, float water_level, int warm, ow::BuoyancyPoint *pts, ow::BuoyancyResult *results) {
    const ow::SurfaceScales sc = scales_of(map_scales, cascades);
    const ow::QueryParams qp = query_params(max_iterations, tolerance, falloff, cx, cz);
    ow::BuoyancyParams bp;
    bp.density = density;
    bp.rho_g = rho_g;
    bp.water_level = water_level;
    bp.warm_start = warm;
    bp.water_velocity = 1;
    for (int i = 0; i < num_points; ++i) {
        ow::BuoyancyPoint prev;
        if (warm) {
            prev = pts[i];
        } else {
            prev.world[0] = prev.world[2] = prev.p[0] = prev.p[1] = 0.0f;
            prev.converged = 0;
        }
        pts[i] = ow::buoyancy_point_moving((const ow::u16x4 *)disp, (const ow::u16x4 *)vel, n, cascades, sc, qp, bp, bodies, num_bodies, hull, i, prev);
    }
    static ow::BodySum lane[64], next[64];
    for (int b = 0; b < num_bodies; ++b) {
        for (int l = 0; l < 64; ++l) lane[l] = ow::body_sum_lane(bodies[b], b, hull, pts, num_points, l);
        for (int m = 32; m >= 1; m >>= 1) {
            for (int l = 0; l < 64; ++l) next[l] = ow::body_sum_combine(lane[l], lane[l ^ m]);
            memcpy(lane, next, sizeof(lane));
        }
        results[b] = ow::body_result(lane[0], bodies[b]);
    }
}

}  // extern "C"

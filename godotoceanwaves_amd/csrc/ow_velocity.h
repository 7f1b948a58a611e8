// ow_velocity.h -- per-point consumer arithmetic over the velocity layers V (ow_velocity_kernels.h): the velocity of the rendered surface
// above a world point (ow_query_velocity) and the moving water of the buoyancy model (OW_BUOYANCY_WATER_VELOCITY).
//
// The rendered vertex of mesh point p is p + f(p) D(p, t) with D = sum_i scales_i.z * bilinear(disp_i, p * scales_i.xy).xyz
// (water.gdshader:27-39); its velocity is f(p) sum_i scales_i.z * bilinear(V_i, p * scales_i.xy).xyz, since V_i = dD_i/dt texel by texel
// and the bilinear weights do not depend on t.  Taken at the query's solved p it is the water's velocity at the surface above (x, z).  A
// point below the surface gets the surface's velocity: there is no decay with depth (the e^{k y} of deep water is not modelled).
//
// Compiles as device code (ow_consumer.hip, -ffp-contract=off) and as plain C++ (tests/velocity/, g++ -ffp-contract=off), like
// ow_surface.h: FP32 adds and multiplies in a fixed cascade order, the same bits in both builds.
#pragma once

#include "ow_buoyancy.h"

namespace ow {

// layout-identical to ow_surface_velocity in include/ocean_waves.h
struct SurfaceVelocity {
    float velocity[3];
    float height;
    float p[2];
    int32_t converged;
    uint32_t reserved;
};
static_assert(sizeof(SurfaceVelocity) == 32, "record layout");

// f * sum_i scales_i.z * bilinear(V_i, (x, z) * scales_i.xy).xyz, the sum in cascade order from 0 (bilinear: ow_surface.h, the taps of
// the displacement lookup)
OW_DEV void velocity_sum(const u16x4 *vel, int n, int cascades, const SurfaceScales &scales, float x, float z, float f, float v[3]) {
    float s[3] = {0.0f, 0.0f, 0.0f};
    const size_t plane = (size_t)n * n;
    for (int c = 0; c < cascades; ++c) {
        const float sx = scales.s[c][0], sy = scales.s[c][1], sz = scales.s[c][2];
        float d[4];
        bilinear(vel + c * plane, n, make_tap(x * sx, z * sy, n), d);
        for (int k = 0; k < 3; ++k) s[k] += d[k] * sz;
    }
    for (int k = 0; k < 3; ++k) v[k] = f * s[k];
}

// One record of ow_query_velocity at world point (qx, qz): p, converged and height are ow_query_surface's (query_solve from q, one
// displacement tap per cascade for the height: the bits of ow_surface_query.height, as the buoyancy model takes them).
OW_DEV SurfaceVelocity velocity_point(const u16x4 *disp, const u16x4 *vel, int n, int cascades, const SurfaceScales &scales, const QueryParams &qp,
                                      float qx, float qz) {
    const QuerySolution sol = query_solve(disp, n, cascades, scales, qp, qx, qz, qx, qz);
    SurfaceVelocity o;
    velocity_sum(vel, n, cascades, scales, sol.p[0], sol.p[1], sol.e.f, o.velocity);
    o.height = sol.e.f * displacement_y(disp, n, cascades, scales, sol.p[0], sol.p[1]);
    o.p[0] = sol.p[0];
    o.p[1] = sol.p[1];
    o.converged = (sol.finite && sol.e.r <= qp.tolerance) ? 1 : 0;
    o.reserved = 0u;
    return o;
}

// the water of the buoyancy model with OW_BUOYANCY_WATER_VELOCITY (ow_buoyancy.h buoyancy_point_in)
struct MovingWater {
    static constexpr bool kMoving = true;
    const u16x4 *vel;
    int n, cascades;
    const SurfaceScales *scales;
    OW_DEV void operator()(float px, float pz, float f, float *vw) const { velocity_sum(vel, n, cascades, *scales, px, pz, f, vw); }
};

OW_DEV BuoyancyPoint buoyancy_point_moving(const u16x4 *disp, const u16x4 *vel, int n, int cascades, const SurfaceScales &scales,
                                           const QueryParams &qp, const BuoyancyParams &bp, const BuoyancyBody *bodies, int num_bodies,
                                           const HullPoint *hull, int i, const BuoyancyPoint &prev) {
    const MovingWater water{vel, n, cascades, &scales};
    return buoyancy_point_in(disp, n, cascades, scales, qp, bp, bodies, num_bodies, hull, i, prev, water);
}

}  // namespace ow

// bodies_harness.cpp -- godotoceanwaves_amd/csrc/ow_rigid.h over ow_buoyancy.h compiled as plain C++ (g++ -ffp-contract=off): the substep
// loop of k_bodies_step -- per body the 64 lanes and the xor tree stepped one after the other -- over maps in host memory, and the pieces
// a host loop around ow_buoyancy_async needs (the pose record, the integrator).  Test infrastructure (tests/test_bodies_step.py); the GPU
// states and records are held to these bit for bit.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "ow_velocity.h"
#include "ow_rigid.h"

extern "C" {

int harness_bodies_sizes(int *sizes) {
    sizes[0] = (int)sizeof(ow::RigidBody);
    sizes[1] = (int)offsetof(ow::RigidBody, orientation);
    sizes[2] = (int)offsetof(ow::RigidBody, mass);
    sizes[3] = (int)offsetof(ow::RigidBody, inverse_inertia);
    sizes[4] = (int)offsetof(ow::RigidBody, applied_torque);
    sizes[5] = (int)offsetof(ow::RigidBody, linear_drag);
    sizes[6] = (int)offsetof(ow::RigidBody, point_offset);
    return 0;
}

// what ow_bodies_create / ow_bodies_set_state leave on the device: pose records, lowered flags, zeroed point records
void harness_bodies_pose(const ow::RigidBody *state, int num_bodies, int num_points, ow::BuoyancyBody *records, ow::BuoyancyPoint *pts, int32_t *flags) {
    for (int b = 0; b < num_bodies; ++b) {
        records[b] = ow::rigid_pose(state[b], ow::rigid_ok(state[b]));
        flags[b] = 0;
    }
    if (num_points > 0) memset(pts, 0, (size_t)num_points * sizeof(ow::BuoyancyPoint));
}

void harness_rigid_pose(const ow::RigidBody *s, ow::BuoyancyBody *record) { *record = ow::rigid_pose(*s, ow::rigid_ok(*s)); }

// a host loop's share of a substep: the result record of ow_buoyancy_async for the pose rigid_pose formed -> the state and the flag
void harness_rigid_finish(ow::RigidBody *s, int32_t *flag, const ow::BuoyancyResult *r, double dt, double gravity) {
    const bool ok = ow::rigid_ok(*s);
    ow::RigidParams rp{dt, gravity};
    if (!ok) {
        *flag = 1;
    } else if (s->mass > 0.0 && *flag == 0) {
        if (!ow::rigid_integrate(*s, *r, rp)) *flag = 1;
    }
}

// `substeps` substeps exactly as k_bodies_step takes them.  vel: the velocity layers (OW_BUOYANCY_WATER_VELOCITY) or NULL.  trace: NULL, or
// substeps x num_bodies result records that receive every substep's results; trace_records likewise the pose records each substep used.
void harness_bodies_step(const uint16_t *disp, const uint16_t *vel, int n, int cascades, const float *map_scales, ow::RigidBody *state, int num_bodies,
                         const ow::HullPoint *hull, int num_points, int max_iterations, float tolerance, int falloff, float cx, float cz, float density,
                         float rho_g, float water_level, int warm, double gravity, double dt, int substeps, ow::BuoyancyBody *records,
                         ow::BuoyancyPoint *pts, ow::BuoyancyResult *results, int32_t *flags, ow::BuoyancyResult *trace, ow::BuoyancyBody *trace_records) {
    ow::SurfaceScales sc;
    memset(&sc, 0, sizeof(sc));
    memcpy(sc.s, map_scales, (size_t)cascades * 4 * sizeof(float));
    ow::QueryParams qp;
    qp.max_iterations = max_iterations;
    qp.tolerance = tolerance;
    qp.falloff = falloff;
    qp.center[0] = cx;
    qp.center[1] = cz;
    ow::BuoyancyParams bp;
    bp.density = density;
    bp.rho_g = rho_g;
    bp.water_level = water_level;
    bp.warm_start = warm;
    bp.water_velocity = vel ? 1 : 0;
    const ow::RigidParams rp{dt, gravity};
    const ow::u16x4 *d = (const ow::u16x4 *)disp, *v = (const ow::u16x4 *)vel;
    static ow::BodySum lane[64], next[64];
    for (int bi = 0; bi < num_bodies; ++bi) {
        ow::RigidBody s = state[bi];
        int32_t flag = flags[bi];
        for (int step = 0; step < substeps; ++step) {
            const bool ok = ow::rigid_ok(s);
            const ow::BuoyancyBody b = ow::rigid_pose(s, ok);
            records[bi] = b;
            if (trace_records) trace_records[(size_t)step * num_bodies + bi] = b;
            for (int l = 0; l < 64; ++l) {
                if (v) {
                    const ow::MovingWater water{v, n, cascades, &sc};
                    lane[l] = ow::rigid_lane(d, n, cascades, sc, qp, bp, b, bi, s.point_offset, s.point_count, hull, pts, num_points, l, water);
                } else {
                    lane[l] = ow::rigid_lane(d, n, cascades, sc, qp, bp, b, bi, s.point_offset, s.point_count, hull, pts, num_points, l, ow::StillWater{});
                }
            }
            for (int m = 32; m >= 1; m >>= 1) {
                for (int l = 0; l < 64; ++l) next[l] = ow::body_sum_combine(lane[l], lane[l ^ m]);
                memcpy(lane, next, sizeof(lane));
            }
            const ow::BuoyancyResult r = ow::rigid_finish(s, ok, flag, lane[0], b, rp);
            results[bi] = r;
            if (trace) trace[(size_t)step * num_bodies + bi] = r;
        }
        records[bi] = ow::rigid_pose(s, ow::rigid_ok(s));
        state[bi] = s;
        flags[bi] = flag;
    }
}

}  // extern "C"

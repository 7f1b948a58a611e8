// ow_buoyancy.h -- buoyancy and drag of rigid bodies on the rendered surface (include/ocean_waves.h ow_buoyancy): the per-point evaluation
// over a body's hull points and the fixed order in which a body's points are summed.
//
// Compiles as device code (ow_consumer.hip, built with -ffp-contract=off) and as plain C++ (tests/buoyancy/, g++ -ffp-contract=off), like
// ow_surface.h: per point every operation is an IEEE-754 FP32 add, multiply, divide, square root, min / max or compare; per body every
// operation is an FP64 add, multiply or divide in the order below.  Both builds produce the same bits.
//
// The model.  Body b has the pose T_b = (B, o) in Godot's Transform3D layout (transform[0..8] = the three rows of the basis B,
// transform[9..11] = the origin o; world = B * local + o), a linear velocity v, an angular velocity w (world axes, rad/s) and drag
// coefficients k_lin (1/s) and k_quad (1/m).  It owns the hull points [point_offset, point_offset + point_count).  Hull point i has a
// local position, a volume V_i >= 0 (m^3), a half height h_i >= 0 (m) and the index of its body.  Per point, in FP32:
//   r_i  = B * local_i                           row k: (B[k][0] * l.x + B[k][1] * l.y) + B[k][2] * l.z -- the lever arm, not w - o
//   w_i  = r_i + o
//   p    solves p + f(p) D_xz(p) = (w.x, w.z)    ow_surface.h query_solve, from p0 = q (cold) or p_prev + (q - q_prev) (warm start:
//                                                from the point's previous record if that converged, and only where p0 is finite and
//                                                within kWarmStartReach of q)
//   H_i  = f(p) * D_y(p)                         the same bits as ow_surface_query.height: one displacement tap per cascade
//   d_i  = (water_level + H_i) - w.y             depth below the surface (negative above it)
//   s_i  = clamp((d_i + h_i) / (h_i + h_i), 0, 1), or (d_i > 0 ? 1 : 0) where h_i = 0     submerged fraction
//   sv_i = V_i * s_i                             submerged volume
//   u_i  = v + w x r_i                           the point's velocity relative to the water; the water is taken at rest, or, with
//                                                OW_BUOYANCY_WATER_VELOCITY, u_i = (v + w x r_i) - v_w with v_w the velocity of the
//                                                rendered surface above the point (ow_velocity.h velocity_sum at p; a point below the
//                                                surface gets the surface's velocity: there is no decay with depth)
//   c_i  = density * sv_i,  m_i = k_quad * |u_i|  (|u| = sqrt((u.x^2 + u.y^2) + u.z^2))
//   drag = c_i * (k_lin * u_i + m_i * u_i)       per component
//   F_i  = (-drag.x, (density * gravity) * sv_i - drag.y, -drag.z)
// A point is INVALID -- its record is zeros with body = -1, it contributes nothing and is counted -- when its body index is outside
// [0, num_bodies), it lies outside the range its body names, any input of it or of its body is not finite, V_i or h_i is negative, or
// its world position, depth or force is not finite, or its world position lies beyond what the query solves (ow_surface.h query_solve: 3e38,
// or kCoordMax tile lengths of a cascade).  No input produces NaN or Inf in any output.
//
// Per body, in FP64, one 64-lane wave: lane l visits the points off + l, off + l + 64, ... of its range in sequence (indices outside
// [0, num_points) are counted invalid and not read; records whose body is not b are counted invalid) and adds, for each valid point,
//   F += F_i,  T += r_i x F_i (components (r.y F.z - r.z F.y, r.z F.x - r.x F.z, r.x F.y - r.y F.x)),  SV += sv_i,  M += sv_i * r_i
// (each FP32 value widened first).  The 64 lanes are combined by the xor tree 32, 16, 8, 4, 2, 1: at each step every lane adds its
// partner's partial to its own (own + partner).  The result: force = F, torque = T (about o, world axes), submerged_volume = SV,
// center_of_buoyancy = o + M / SV (o where SV = 0, or 0 where o is not finite), rounded to FP32 (saturating at +-FLT_MAX); the wetted
// (s_i > 0), unconverged and invalid point counts; the largest residual of a valid point.  No floating-point atomics.
#pragma once

#include "ow_surface.h"

namespace ow {

// layout-identical to ow_buoyancy_body / ow_hull_point / ow_buoyancy_point / ow_buoyancy_result in include/ocean_waves.h
struct BuoyancyBody {
    float transform[12];
    float linear_velocity[3];
    float angular_velocity[3];
    int32_t point_offset, point_count;
    float linear_drag, quadratic_drag;
    uint32_t reserved[2];
};
struct HullPoint {
    float local[3];
    float volume, half_height;
    int32_t body;
    uint32_t reserved[2];
};
struct BuoyancyPoint {
    float world[3];
    float height, depth, submerged;
    float force[3];
    float p[2];
    float residual;
    int32_t iterations, evaluations, converged;
    int32_t body;  // the body the point was counted for; -1: invalid
};
struct BuoyancyResult {
    float force[3], torque[3];
    float submerged_volume;
    float center_of_buoyancy[3];
    int32_t wetted_points, unconverged_points, invalid_points;
    float max_residual;
    uint32_t reserved[2];
};
static_assert(sizeof(BuoyancyBody) == 96 && sizeof(HullPoint) == 32 && sizeof(BuoyancyPoint) == 64 && sizeof(BuoyancyResult) == 64,
              "record layout");

// the model's constants, resolved from ow_buoyancy_options by the runtime
constexpr float kDefaultDensity = 1025.0f;  // sea water, kg/m^3
constexpr float kDefaultGravity = 9.81f;    // wave_generator.gd's G
constexpr float kWarmStartReach = 1000.0f;  // metres: a warm start farther than this from q (stale or foreign records) starts at q
struct BuoyancyParams {
    float density;      // kg/m^3, > 0
    float rho_g;        // density * gravity in FP32
    float water_level;  // metres
    int warm_start;     // 1: start Newton from the lane's previous record
    float gravity;      // m/s^2, as resolved (rho_g = density * gravity); the integrator of ow_rigid.h widens it
    int water_velocity; // 1: drag relative to the moving surface (OW_BUOYANCY_WATER_VELOCITY; the runtime picks the kernel by it)
};

OW_DEV bool finite_f32(float x) { return fabsf(x) <= 3.4028235e38f; }

// r = B * local, row by row
OW_DEV void lever_arm(const BuoyancyBody &b, const float l[3], float r[3]) {
    for (int k = 0; k < 3; ++k) r[k] = (b.transform[3 * k] * l[0] + b.transform[3 * k + 1] * l[1]) + b.transform[3 * k + 2] * l[2];
}

// sum_i D_y,i(p): the .y of the displacement sum sample_point forms, in the same operations (one tap per cascade)
OW_DEV float displacement_y(const u16x4 *disp, int n, int cascades, const SurfaceScales &scales, float x, float z) {
    float y = 0.0f;
    const size_t plane = (size_t)n * n;
    for (int c = 0; c < cascades; ++c) {
        const float sx = scales.s[c][0], sy = scales.s[c][1], sz = scales.s[c][2];
        const Tap t = make_tap(x * sx, z * sy, n);
        float a[4], b[4], cc[4], d[4];
        load_quad(disp + c * plane, n, t, a, b, cc, d);
        const float ux = 1.0f - t.wx, uy = 1.0f - t.wy;
        y += ((a[1] * ux + b[1] * t.wx) * uy + (cc[1] * ux + d[1] * t.wx) * t.wy) * sz;
    }
    return y;
}

OW_DEV BuoyancyPoint invalid_point() {
    BuoyancyPoint o;
    o.world[0] = o.world[1] = o.world[2] = 0.0f;
    o.height = o.depth = o.submerged = 0.0f;
    o.force[0] = o.force[1] = o.force[2] = 0.0f;
    o.p[0] = o.p[1] = 0.0f;
    o.residual = 0.0f;
    o.iterations = o.evaluations = o.converged = 0;
    o.body = -1;
    return o;
}

// The water of the model: at rest (StillWater), or moving with the velocity maps (ow_velocity.h MovingWater: kMoving, and
// water(px, pz, f, vw) writes the surface velocity v_w at the solved point p with falloff f).
struct StillWater {
    static constexpr bool kMoving = false;
    OW_DEV void operator()(float, float, float, float *) const {}
};

// Hull point i.  prev: the lane's record of the previous step (read only with bp.warm_start: world, p, converged; zeros make a cold start).
template <class Water>
OW_DEV BuoyancyPoint buoyancy_point_in(const u16x4 *disp, int n, int cascades, const SurfaceScales &scales, const QueryParams &qp,
                                       const BuoyancyParams &bp, const BuoyancyBody *bodies, int num_bodies, const HullPoint *hull, int i,
                                       const BuoyancyPoint &prev, const Water &water) {
    const HullPoint hp = hull[i];
    const int bi = hp.body;
    if (bi < 0 || bi >= num_bodies) return invalid_point();
    const BuoyancyBody b = bodies[bi];
    if ((int64_t)i < (int64_t)b.point_offset || (int64_t)i >= (int64_t)b.point_offset + (int64_t)b.point_count) return invalid_point();
    bool ok = finite_f32(hp.volume) && finite_f32(hp.half_height) && hp.volume >= 0.0f && hp.half_height >= 0.0f;
    for (int k = 0; k < 12; ++k) ok = ok && finite_f32(b.transform[k]);
    for (int k = 0; k < 3; ++k)
        ok = ok && finite_f32(hp.local[k]) && finite_f32(b.linear_velocity[k]) && finite_f32(b.angular_velocity[k]);
    ok = ok && finite_f32(b.linear_drag) && finite_f32(b.quadratic_drag);
    if (!ok) return invalid_point();
    float r[3], w[3];
    lever_arm(b, hp.local, r);
    for (int k = 0; k < 3; ++k) w[k] = r[k] + b.transform[9 + k];
    if (!(finite_f32(w[0]) && finite_f32(w[1]) && finite_f32(w[2]))) return invalid_point();

    const float qx = w[0], qz = w[2];
    float p0x = qx, p0z = qz;
    if (bp.warm_start && prev.converged == 1) {  // a point that did not converge last step (a fold, or no record yet) starts cold
        const float wx = prev.p[0] + (qx - prev.world[0]), wz = prev.p[1] + (qz - prev.world[2]);
        if (fabsf(wx - qx) <= kWarmStartReach && fabsf(wz - qz) <= kWarmStartReach) {  // false for a non-finite start
            p0x = wx;
            p0z = wz;
        }
    }
    const QuerySolution sol = query_solve(disp, n, cascades, scales, qp, qx, qz, p0x, p0z);
    const float height = sol.e.f * displacement_y(disp, n, cascades, scales, sol.p[0], sol.p[1]);
    const float depth = (bp.water_level + height) - w[1];
    const float h = hp.half_height;
    float s;
    if (h > 0.0f) {
        const float t = (depth + h) / (h + h);
        s = (t > 0.0f) ? ((t < 1.0f) ? t : 1.0f) : 0.0f;  // NaN -> 0
    } else {
        s = depth > 0.0f ? 1.0f : 0.0f;
    }
    const float sv = hp.volume * s;
    const float *v = b.linear_velocity, *om = b.angular_velocity;
    float u[3] = {v[0] + (om[1] * r[2] - om[2] * r[1]), v[1] + (om[2] * r[0] - om[0] * r[2]), v[2] + (om[0] * r[1] - om[1] * r[0])};
    if constexpr (Water::kMoving) {
        float vw[3];
        water(sol.p[0], sol.p[1], sol.e.f, vw);
        for (int k = 0; k < 3; ++k) u[k] = u[k] - vw[k];
    }
    const float un = sqrtf((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
    const float c = bp.density * sv, m = b.quadratic_drag * un;
    float drag[3];
    for (int k = 0; k < 3; ++k) drag[k] = c * (b.linear_drag * u[k] + m * u[k]);

    BuoyancyPoint o;
    o.force[0] = -drag[0];
    o.force[1] = bp.rho_g * sv - drag[1];
    o.force[2] = -drag[2];
    if (!(sol.finite && finite_f32(depth) && finite_f32(o.force[0]) && finite_f32(o.force[1]) && finite_f32(o.force[2]))) return invalid_point();
    o.world[0] = w[0];
    o.world[1] = w[1];
    o.world[2] = w[2];
    o.height = height;
    o.depth = depth;
    o.submerged = s;
    o.p[0] = sol.p[0];
    o.p[1] = sol.p[1];
    o.residual = sol.e.r;
    o.iterations = sol.iterations;
    o.evaluations = sol.evaluations;
    o.converged = (sol.finite && sol.e.r <= qp.tolerance) ? 1 : 0;
    o.body = bi;
    return o;
}
OW_DEV BuoyancyPoint buoyancy_point(const u16x4 *disp, int n, int cascades, const SurfaceScales &scales, const QueryParams &qp,
                                    const BuoyancyParams &bp, const BuoyancyBody *bodies, int num_bodies, const HullPoint *hull, int i,
                                    const BuoyancyPoint &prev) {
    return buoyancy_point_in(disp, n, cascades, scales, qp, bp, bodies, num_bodies, hull, i, prev, StillWater{});
}

// ---- the per-body sum ----------------------------------------------------------------------------------------------------------------

struct BodySum {
    double F[3], T[3], SV, M[3];
    int wetted, unconverged, invalid;
    float max_residual;
};

OW_DEV BodySum body_sum_zero() {
    BodySum a;
    for (int k = 0; k < 3; ++k) a.F[k] = a.T[k] = a.M[k] = 0.0;
    a.SV = 0.0;
    a.wetted = a.unconverged = a.invalid = 0;
    a.max_residual = 0.0f;
    return a;
}

// own + partner: one step of the xor tree (IEEE addition commutes, so both lanes of a pair hold the same bits afterwards)
OW_DEV BodySum body_sum_combine(const BodySum &a, const BodySum &b) {
    BodySum s;
    for (int k = 0; k < 3; ++k) {
        s.F[k] = a.F[k] + b.F[k];
        s.T[k] = a.T[k] + b.T[k];
        s.M[k] = a.M[k] + b.M[k];
    }
    s.SV = a.SV + b.SV;
    s.wetted = a.wetted + b.wetted;
    s.unconverged = a.unconverged + b.unconverged;
    s.invalid = a.invalid + b.invalid;
    s.max_residual = a.max_residual > b.max_residual ? a.max_residual : b.max_residual;
    return s;
}

// one valid record added to a lane's sums: the operations and their order (shared with ow_rigid.h's fused substep)
OW_DEV void body_sum_add(BodySum &a, const BuoyancyBody &b, const HullPoint &hp, const BuoyancyPoint &rec) {
    float r[3];
    lever_arm(b, hp.local, r);  // the bits the point kernel used
    const double rx = r[0], ry = r[1], rz = r[2], fx = rec.force[0], fy = rec.force[1], fz = rec.force[2];
    const double svi = (double)(hp.volume * rec.submerged);
    a.F[0] += fx;
    a.F[1] += fy;
    a.F[2] += fz;
    a.T[0] += ry * fz - rz * fy;
    a.T[1] += rz * fx - rx * fz;
    a.T[2] += rx * fy - ry * fx;
    a.SV += svi;
    a.M[0] += svi * rx;
    a.M[1] += svi * ry;
    a.M[2] += svi * rz;
    a.wetted += rec.submerged > 0.0f ? 1 : 0;
    a.unconverged += rec.converged ? 0 : 1;
    if (rec.residual > a.max_residual) a.max_residual = rec.residual;
}

// lane l's share of body bi: the points off + l, off + l + 64, ... in sequence
OW_DEV BodySum body_sum_lane(const BuoyancyBody &b, int bi, const HullPoint *hull, const BuoyancyPoint *pts, int num_points, int lane) {
    BodySum a = body_sum_zero();
    if (b.point_count <= 0) return a;
    const int64_t off = b.point_offset, end = off + (int64_t)b.point_count;
    const int64_t lo = off > 0 ? off : 0, hi = end < (int64_t)num_points ? end : (int64_t)num_points;
    if (lane == 0) a.invalid = (int)((int64_t)b.point_count - (hi > lo ? hi - lo : 0));  // outside [0, num_points): never read
    int64_t i = off + lane;
    if (i < lo) i += (lo - i + 63) / 64 * 64;
    for (; i < hi; i += 64) {
        const BuoyancyPoint rec = pts[i];
        if (rec.body != bi) {
            ++a.invalid;
            continue;
        }
        body_sum_add(a, b, hull[i], rec);
    }
    return a;
}

OW_DEV float saturate_f32(double x) { return x > 3.4028234663852886e38 ? 3.4028235e38f : (x < -3.4028234663852886e38 ? -3.4028235e38f : (float)x); }

OW_DEV BuoyancyResult body_result(const BodySum &a, const BuoyancyBody &b) {
    BuoyancyResult o;
    for (int k = 0; k < 3; ++k) {
        o.force[k] = saturate_f32(a.F[k]);
        o.torque[k] = saturate_f32(a.T[k]);
    }
    o.submerged_volume = saturate_f32(a.SV);
    const bool o_finite = finite_f32(b.transform[9]) && finite_f32(b.transform[10]) && finite_f32(b.transform[11]);
    for (int k = 0; k < 3; ++k) {
        const double ok = o_finite ? (double)b.transform[9 + k] : 0.0;
        o.center_of_buoyancy[k] = saturate_f32(a.SV > 0.0 ? ok + a.M[k] / a.SV : ok);
    }
    o.wetted_points = a.wetted;
    o.unconverged_points = a.unconverged;
    o.invalid_points = a.invalid;
    o.max_residual = a.max_residual;
    o.reserved[0] = o.reserved[1] = 0;
    return o;
}

}  // namespace ow

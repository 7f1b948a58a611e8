// ow_rigid.h -- floating rigid bodies stepped from the buoyancy forces (include/ocean_waves.h ow_bodies_step): the FP64 state of a body, the
// pose record formed from it, the lane's share of a substep (its hull points evaluated and summed as it goes) and the integrator.
//
// Compiles as device code (ow_consumer.hip, built with -ffp-contract=off) and as plain C++ (tests/bodies/, g++ -ffp-contract=off), like
// ow_buoyancy.h: every operation below is an IEEE-754 FP64 add, multiply, divide, square root or compare (no sin / cos, no fused
// multiply-add), in the order written here.  Both builds produce the same bits.  The per-point evaluation (buoyancy_point /
// buoyancy_point_moving), the per-body sum's order (body_sum_lane's), the xor tree (body_sum_combine) and body_result are ow_buoyancy.h's,
// unchanged: the ow_buoyancy_point and ow_buoyancy_result records of a substep are the bits ow_buoyancy_async writes for that pose.
//
// State per body (RigidBody = ow_rigid_body, FP64): position o, orientation q (a unit quaternion in Godot's x, y, z, w order; world =
// R(q) * local + o), linear velocity v and angular velocity w (world axes), mass m, the inverse principal inertia Iinv[3] in body axes (0
// locks that axis), a constant applied force Fa and torque Ta (world axes), the two drag coefficients and the hull range of
// ow_buoyancy_body.
//
// One substep of length dt:
//   1. the pose record (rigid_pose): with x, y, z, w = q,
//        R = [1 - 2 (yy + zz), 2 (xy - zw), 2 (xz + yw);  2 (xy + zw), 1 - 2 (xx + zz), 2 (yz - xw);  2 (xz - yw), 2 (yz + xw), 1 - 2 (xx + yy)]
//      in FP64, narrowed to FP32 into transform[0..8] (saturating at +-FLT_MAX, as o, v and w are); the drag coefficients and the hull range
//      copied.  The record is written.
//   2. lane l of the body's 64-lane wave evaluates the hull points off + l, off + l + 64, ... in sequence (rigid_lane), writes each record
//      and adds it to its partial sums at once -- body_sum_lane's order and operations, so the sums have its bits without the records making
//      a round trip; the xor tree 32 .. 1 and body_result follow.  The result record is written.
//   3. semi-implicit Euler from the result record as written (its FP32 values widened), rigid_integrate:
//        a_k  = (F_k + Fa_k) / m,  a_y = a_y + (-g);                       v_k += dt * a_k
//        tau  = T + Ta;  b_j = ((R_0j tau_0 + R_1j tau_1) + R_2j tau_2) * Iinv_j;    w_i += dt * ((R_i0 b_0 + R_i1 b_1) + R_i2 b_2)
//        o_k += dt * v_k                                                   (the new v)
//        d    = (w, 0) (x) q = (wx qw + wy qz - wz qy,  wy qw + wz qx - wx qz,  wz qw + wx qy - wy qx,  -((wx qx + wy qy) + wz qz))
//        q_k += (dt * 0.5) * d_k;  q_k /= sqrt((qx^2 + qy^2) + (qz^2 + qw^2))   (the new w; R above is that of the old q)
//      THERE IS NO GYROSCOPIC TERM (w x I w is dropped, as in examples/buoyancy_host.c): a freely tumbling asymmetric body keeps its
//      angular velocity instead of precessing.  On the water the drag torque dominates it.
//    Steps 1 and 3 have a twin in exact rational arithmetic written from this comment (tests/rigid_twin.py), which both builds are held to.
//
// Bodies that are not integrated.  mass <= 0: kinematic -- its record, points and result are computed, its state stays.  A body whose state
// or inputs are not finite, or whose quaternion has no length (rigid_ok), is FAULTED: its record is the null record (identity basis, zeros,
// an empty hull range -- its hull points' records are the invalid record, its result zeros), its state is left as the caller gave it and it
// is flagged.  A body whose state would become non-finite in a substep keeps the state it had (the last finite one) and is flagged; a
// flagged body is evaluated like a kinematic one from then on, until its state is set again.  No input puts NaN or Inf into a pose, point
// or result record, nor into the state of a body whose state was finite.
#pragma once

#include "ow_buoyancy.h"

namespace ow {

// layout-identical to ow_rigid_body in include/ocean_waves.h
struct RigidBody {
    double position[3];
    double orientation[4];
    double linear_velocity[3];
    double angular_velocity[3];
    double mass;
    double inverse_inertia[3];
    double applied_force[3];
    double applied_torque[3];
    float linear_drag, quadratic_drag;
    int32_t point_offset, point_count;
    uint32_t reserved[2];
};
static_assert(sizeof(RigidBody) == 208, "record layout");

struct RigidParams {
    double dt;       // seconds, > 0
    double gravity;  // m/s^2: the FP32 gravity of ow_buoyancy_options as resolved, widened
};

OW_DEV bool finite_f64(double x) { return (x < 0.0 ? -x : x) <= 1.7976931348623157e308; }

// every field finite and a quaternion of non-zero, finite squared length
OW_DEV bool rigid_ok(const RigidBody &s) {
    bool ok = finite_f64(s.mass) && finite_f32(s.linear_drag) && finite_f32(s.quadratic_drag);
    for (int k = 0; k < 3; ++k)
        ok = ok && finite_f64(s.position[k]) && finite_f64(s.linear_velocity[k]) && finite_f64(s.angular_velocity[k]) &&
             finite_f64(s.inverse_inertia[k]) && finite_f64(s.applied_force[k]) && finite_f64(s.applied_torque[k]);
    for (int k = 0; k < 4; ++k) ok = ok && finite_f64(s.orientation[k]);
    const double *q = s.orientation;
    const double n2 = (q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]);
    return ok && finite_f64(n2) && n2 > 0.0;
}

// the rows of R(q)
OW_DEV void rigid_basis(const double q[4], double R[9]) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, xw = x * w, yw = y * w, zw = z * w;
    R[0] = 1.0 - 2.0 * (yy + zz);
    R[1] = 2.0 * (xy - zw);
    R[2] = 2.0 * (xz + yw);
    R[3] = 2.0 * (xy + zw);
    R[4] = 1.0 - 2.0 * (xx + zz);
    R[5] = 2.0 * (yz - xw);
    R[6] = 2.0 * (xz - yw);
    R[7] = 2.0 * (yz + xw);
    R[8] = 1.0 - 2.0 * (xx + yy);
}

// step 1: the ow_buoyancy_body record of state s (ok: rigid_ok(s); the null record otherwise)
OW_DEV BuoyancyBody rigid_pose(const RigidBody &s, bool ok) {
    BuoyancyBody b;
    for (int k = 0; k < 12; ++k) b.transform[k] = 0.0f;
    b.transform[0] = b.transform[4] = b.transform[8] = 1.0f;
    for (int k = 0; k < 3; ++k) b.linear_velocity[k] = b.angular_velocity[k] = 0.0f;
    b.point_offset = s.point_offset;
    b.point_count = 0;
    b.linear_drag = b.quadratic_drag = 0.0f;
    b.reserved[0] = b.reserved[1] = 0u;
    if (!ok) return b;
    double R[9];
    rigid_basis(s.orientation, R);
    for (int k = 0; k < 9; ++k) b.transform[k] = saturate_f32(R[k]);
    for (int k = 0; k < 3; ++k) {
        b.transform[9 + k] = saturate_f32(s.position[k]);
        b.linear_velocity[k] = saturate_f32(s.linear_velocity[k]);
        b.angular_velocity[k] = saturate_f32(s.angular_velocity[k]);
    }
    b.point_count = s.point_count;
    b.linear_drag = s.linear_drag;
    b.quadratic_drag = s.quadratic_drag;
    return b;
}

// Hull point i of body bi, whose record b the lane holds in registers: buoyancy_point_in on a one-body, one-point view (the body at index 0
// with the range [0, 1) or, where i lies outside b's range, the empty one), so that its operations are the point kernel's on the arrays.
template <class Water>
OW_DEV BuoyancyPoint rigid_point(const u16x4 *disp, int n, int cascades, const SurfaceScales &scales, const QueryParams &qp,
                                 const BuoyancyParams &bp, const BuoyancyBody &b, int bi, const HullPoint *hull, int64_t i,
                                 const BuoyancyPoint &prev, const Water &water) {
    HullPoint hp = hull[i];
    if (hp.body != bi) return invalid_point();
    BuoyancyBody one = b;
    one.point_offset = 0;
    one.point_count = (i >= (int64_t)b.point_offset && i < (int64_t)b.point_offset + (int64_t)b.point_count) ? 1 : 0;
    hp.body = 0;
    BuoyancyPoint o = buoyancy_point_in(disp, n, cascades, scales, qp, bp, &one, 1, &hp, 0, prev, water);
    if (o.body == 0) o.body = bi;
    return o;
}

// step 2, lane `lane` of body bi: the hull points [off, off + count) of the body's state that are the lane's, in sequence -- each evaluated
// against the record b, written to pts[i] (after its previous record has been read, with bp.warm_start) and, where b holds it, added to the
// lane's sums by body_sum_lane's operations in body_sum_lane's order.  Indices outside [0, num_points) are counted, never touched.
template <class Water>
OW_DEV BodySum rigid_lane(const u16x4 *disp, int n, int cascades, const SurfaceScales &scales, const QueryParams &qp, const BuoyancyParams &bp,
                          const BuoyancyBody &b, int bi, int32_t off32, int32_t count, const HullPoint *hull, BuoyancyPoint *pts, int num_points,
                          int lane, const Water &water) {
    BodySum a = body_sum_zero();
    if (count <= 0) return a;
    const int64_t off = off32, end = off + (int64_t)count;
    const int64_t lo = off > 0 ? off : 0, hi = end < (int64_t)num_points ? end : (int64_t)num_points;
    const bool summed = b.point_count > 0;  // the null record sums nothing (body_sum_lane's first line)
    if (lane == 0 && summed) a.invalid = (int)((int64_t)count - (hi > lo ? hi - lo : 0));
    int64_t i = off + lane;
    if (i < lo) i += (lo - i + 63) / 64 * 64;
    for (; i < hi; i += 64) {
        BuoyancyPoint prev;
        if (bp.warm_start) {
            prev = pts[i];
        } else {
            prev.world[0] = prev.world[2] = prev.p[0] = prev.p[1] = 0.0f;
            prev.converged = 0;
        }
        const BuoyancyPoint rec = rigid_point(disp, n, cascades, scales, qp, bp, b, bi, hull, i, prev, water);
        pts[i] = rec;
        if (!summed) continue;
        if (rec.body != bi) {
            ++a.invalid;
            continue;
        }
        body_sum_add(a, b, hull[i], rec);  // body_sum_lane's own accumulation
    }
    return a;
}

// step 3: s advanced by one substep from the result record r.  Returns false, and leaves s as it was, where the new state is not finite.
OW_DEV bool rigid_integrate(RigidBody &s, const BuoyancyResult &r, const RigidParams &rp) {
    const double dt = rp.dt;
    double R[9];
    rigid_basis(s.orientation, R);
    double v[3], w[3], o[3], q[4];
    for (int k = 0; k < 3; ++k) {
        double a = ((double)r.force[k] + s.applied_force[k]) / s.mass;
        if (k == 1) a = a + (-rp.gravity);
        v[k] = s.linear_velocity[k] + dt * a;
    }
    double tau[3], b[3];
    for (int k = 0; k < 3; ++k) tau[k] = (double)r.torque[k] + s.applied_torque[k];
    for (int j = 0; j < 3; ++j) b[j] = ((R[j] * tau[0] + R[3 + j] * tau[1]) + R[6 + j] * tau[2]) * s.inverse_inertia[j];
    for (int i = 0; i < 3; ++i) w[i] = s.angular_velocity[i] + dt * ((R[3 * i] * b[0] + R[3 * i + 1] * b[1]) + R[3 * i + 2] * b[2]);
    for (int k = 0; k < 3; ++k) o[k] = s.position[k] + dt * v[k];
    const double qx = s.orientation[0], qy = s.orientation[1], qz = s.orientation[2], qw = s.orientation[3];
    const double d[4] = {w[0] * qw + w[1] * qz - w[2] * qy, w[1] * qw + w[2] * qx - w[0] * qz, w[2] * qw + w[0] * qy - w[1] * qx,
                         -((w[0] * qx + w[1] * qy) + w[2] * qz)};
    const double h = dt * 0.5;
    for (int k = 0; k < 4; ++k) q[k] = s.orientation[k] + h * d[k];
    const double len = sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
    for (int k = 0; k < 4; ++k) q[k] = q[k] / len;
    bool ok = true;
    for (int k = 0; k < 3; ++k) ok = ok && finite_f64(v[k]) && finite_f64(w[k]) && finite_f64(o[k]);
    for (int k = 0; k < 4; ++k) ok = ok && finite_f64(q[k]);
    if (!ok) return false;
    for (int k = 0; k < 3; ++k) {
        s.linear_velocity[k] = v[k];
        s.angular_velocity[k] = w[k];
        s.position[k] = o[k];
    }
    for (int k = 0; k < 4; ++k) s.orientation[k] = q[k];
    return true;
}

// What a body's wave does with the combined sums (every lane holds the same): the result record, then the integration where the body is
// dynamic, sound and not flagged.  flag: the body's fault flag, raised where the step is refused.  Returns the result record.
OW_DEV BuoyancyResult rigid_finish(RigidBody &s, bool ok, int32_t &flag, const BodySum &a, const BuoyancyBody &b, const RigidParams &rp) {
    const BuoyancyResult r = body_result(a, b);
    if (!ok) {
        flag = 1;
    } else if (s.mass > 0.0 && flag == 0) {
        if (!rigid_integrate(s, r, rp)) flag = 1;
    }
    return r;
}

}  // namespace ow

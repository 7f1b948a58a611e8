// ow_surface.h -- per-point consumer arithmetic over the two RGBA16F array textures: what the water and
// sea-spray shaders read at a world point (sample_point, the body of k_sample_surface), and where the water IS above a world point
// (query_point: the rendered vertex p + f(p) D(p) that lands on (x, z), found by damped Newton).
//
// Compiles as device code (ow_consumer.hip, built with -ffp-contract=off) and as plain C++ (tests/query/, g++ -ffp-contract=off), like
// ow_device.h: every operation is an IEEE-754 FP32 add, multiply, divide or square root, a floor, a min, a max or a compare, and the one
// conversion to an integer (wrap_texel) has an operand in [0, N), so both builds produce the same bits for every input.  There is no library exp(): the distance falloff uses exp_f32 below, written out in those operations.
#pragma once

#include "ow_device.h"

namespace ow {

// SurfaceSample / SurfaceQuery are layout-identical to ow_surface_sample / ow_surface_query in include/ocean_waves.h
struct SurfaceScales {
    float s[8][4];  // map_scales[i] = (1/tile_length.x, 1/tile_length.y, displacement_scale, normal_scale), water.gd:105-109
};
struct SurfaceSample {
    float displacement[3];
    float gradient[2];
    float gradient_scaled[2];
    float foam;
    float normal_factor, foam_factor, scale_factor;
    int32_t spray_active;
    float gradient_fragment[2];
    float foam_fragment;
    float reserved;
};
struct SurfaceQuery {
    float p[2];
    float residual;
    int32_t iterations, evaluations, converged;
    float falloff, height;
    float normal[3];
    float world_xz[2];
    int32_t reserved[3];
    SurfaceSample sample;
};
static_assert(sizeof(SurfaceSample) == 64 && sizeof(SurfaceQuery) == 128, "record layout");

constexpr int kQueryDefaultIterations = 16;
constexpr int kQueryMaxIterations = 64;
constexpr float kQueryDefaultTolerance = 1e-3f;
// the solver's settings, resolved from ow_query_options by the runtime
struct QueryParams {
    int max_iterations;  // 1 .. kQueryMaxIterations
    float tolerance;     // metres, > 0
    int falloff;         // 1: f(p) = water.gdshader:29's distance factor around center; 0: f = 1
    float center[2];     // CAMERA_POSITION_WORLD.xz
};

struct Tap {
    int r0, r1, c0, c1;
    float wx, wy;
};

// x0 mod N for an integer-valued x0 of any magnitude, in float: N is a power of two, so x0 / N, its floor and the product back are
// exact, and the difference is an integer in [0, N) (0 from 2^24 N on, where every float is a multiple of N).  Equal to (int)x0 & (N - 1)
// wherever that conversion is defined; unlike it, defined -- and the same on the device and on the host -- for every finite x0.
OW_DEV int wrap_texel(float x0, float fn) { return (int)(x0 - fn * floorf(x0 * (1.0f / fn))); }

// A normalised texture coordinate (in tiles) is used up to kCoordMax in magnitude: u N - 0.5 is then finite for every map size, so a
// lookup never forms Inf - Inf.  sample_point clamps to it (a point further out reads texel 0 with weight 0, as every coordinate from
// 2^24 tiles on does); query_solve treats a q beyond it like a non-finite q.
constexpr float kCoordMax = 1.0e34f;
OW_DEV float clamp_coord(float u) { return fminf(fmaxf(u, -kCoordMax), kCoordMax); }  // a NaN reads as -kCoordMax

// texel coordinates and weights of one bilinear lookup at normalised (u, v), |u|, |v| <= kCoordMax; u runs along columns
OW_DEV Tap make_tap(float u, float v, int n) {
    const float fn = (float)n;
    const float fx = u * fn - 0.5f, fy = v * fn - 0.5f;
    const float x0 = floorf(fx), y0 = floorf(fy);
    Tap t;
    t.wx = fx - x0;
    t.wy = fy - y0;
    const int mask = n - 1;  // N is a power of two
    t.c0 = wrap_texel(x0, fn);
    t.c1 = (t.c0 + 1) & mask;
    t.r0 = wrap_texel(y0, fn);
    t.r1 = (t.r0 + 1) & mask;
    return t;
}

// the four texels of a tap: a = (r0, c0), b = (r0, c1), c = (r1, c0), d = (r1, c1).  Columns c0 and c0 + 1 are adjacent in a row, so
// a row's pair is one 16-byte load; only a tap whose c0 is the last column wraps to column 0 and takes two 8-byte loads per row.
OW_DEV void load_quad(const u16x4 *layer, int n, const Tap &t, float a[4], float b[4], float c[4], float d[4]) {
    const u16x4 *row0 = layer + (size_t)t.r0 * n, *row1 = layer + (size_t)t.r1 * n;
#if OW_DEVICE_BUILD
    typedef uint32_t u32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));  // a texel is 8-byte aligned
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    typedef float f8 __attribute__((ext_vector_type(8)));
    f8 v0, v1;
    if (t.c1 == t.c0 + 1) {  // one global_load_dwordx4 per row
        v0 = __builtin_convertvector(__builtin_bit_cast(h8, *(const u32x4_a8 *)(row0 + t.c0)), f8);
        v1 = __builtin_convertvector(__builtin_bit_cast(h8, *(const u32x4_a8 *)(row1 + t.c0)), f8);
    } else {
        typedef uint16_t u16x8 __attribute__((ext_vector_type(8)));
        typedef uint16_t u16x4v __attribute__((ext_vector_type(4)));
        const u16x4v qa = __builtin_bit_cast(u16x4v, row0[t.c0]), qb = __builtin_bit_cast(u16x4v, row0[t.c1]);
        const u16x4v qc = __builtin_bit_cast(u16x4v, row1[t.c0]), qd = __builtin_bit_cast(u16x4v, row1[t.c1]);
        v0 = __builtin_convertvector(__builtin_bit_cast(h8, (u16x8)__builtin_shufflevector(qa, qb, 0, 1, 2, 3, 4, 5, 6, 7)), f8);
        v1 = __builtin_convertvector(__builtin_bit_cast(h8, (u16x8)__builtin_shufflevector(qc, qd, 0, 1, 2, 3, 4, 5, 6, 7)), f8);
    }
    for (int k = 0; k < 4; ++k) {  // FP16 -> FP32 is exact: any conversion gives these bits
        a[k] = v0[k];
        b[k] = v0[k + 4];
        c[k] = v1[k];
        d[k] = v1[k + 4];
    }
#else
    const u16x4 q[4] = {row0[t.c0], row0[t.c1], row1[t.c0], row1[t.c1]};
    float *out[4] = {a, b, c, d};
    for (int i = 0; i < 4; ++i) {
        out[i][0] = h2f(q[i].x);
        out[i][1] = h2f(q[i].y);
        out[i][2] = h2f(q[i].z);
        out[i][3] = h2f(q[i].w);
    }
#endif
}

OW_DEV void bilinear(const u16x4 *layer, int n, const Tap &t, float out[4]) {
    float a[4], b[4], c[4], d[4];
    load_quad(layer, n, t, a, b, c, d);
    const float ux = 1.0f - t.wx, uy = 1.0f - t.wy;
    for (int k = 0; k < 4; ++k) out[k] = (a[k] * ux + b[k] * t.wx) * uy + (c[k] * ux + d[k] * t.wx) * t.wy;
}

OW_DEV float glsl_mix(float a, float b, float t) { return a * (1.0f - t) + b * t; }

// water.gdshader:41-51 cubic_weights, :53-68 texture_bicubic: cubic B-spline filtering as four bilinear taps
OW_DEV void cubic_weights(float a, float w[4]) {
    const float a2 = a * a, a3 = a2 * a;
    w[0] = (-a3 + a2 * 3.0f - a * 3.0f + 1.0f) / 6.0f;
    w[1] = (a3 * 3.0f - a2 * 6.0f + 4.0f) / 6.0f;
    w[2] = (-a3 * 3.0f + a2 * 3.0f + a * 3.0f + 1.0f) / 6.0f;
    w[3] = a3 / 6.0f;
}
OW_DEV void bicubic(const u16x4 *layer, int n, float u, float v, float out[4]) {
    const float dims = (float)n, dims_inv = 1.0f / dims;
    const float x = u * dims + 0.5f, y = v * dims + 0.5f;
    const float fx = x - floorf(x), fy = y - floorf(y);
    float wx[4], wy[4];
    cubic_weights(fx, wx);
    cubic_weights(fy, wy);
    const float gx0 = wx[0] + wx[1], gx1 = wx[2] + wx[3], gy0 = wy[0] + wy[1], gy1 = wy[2] + wy[3];
    const float hx0 = (wx[1] / gx0 + -1.5f + floorf(x)) * dims_inv, hx1 = (wx[3] / gx1 + 0.5f + floorf(x)) * dims_inv;
    const float hy0 = (wy[1] / gy0 + -1.5f + floorf(y)) * dims_inv, hy1 = (wy[3] / gy1 + 0.5f + floorf(y)) * dims_inv;
    const float wgx = gx0 / (gx0 + gx1), wgy = gy0 / (gy0 + gy1);
    float t_yw[4], t_xw[4], t_yz[4], t_xz[4];
    bilinear(layer, n, make_tap(hx1, hy1, n), t_yw);
    bilinear(layer, n, make_tap(hx0, hy1, n), t_xw);
    bilinear(layer, n, make_tap(hx1, hy0, n), t_yz);
    bilinear(layer, n, make_tap(hx0, hy0, n), t_xz);
    for (int k = 0; k < 4; ++k) out[k] = glsl_mix(glsl_mix(t_yw[k], t_xw[k], wgx), glsl_mix(t_yz[k], t_xz[k], wgx), wgy);
}

// One record of ow_sample_surface at world point (x, z).  kClamp: hold each cascade's coordinate to kCoordMax (any x and z, the entry
// point's case); without it the caller vouches for that (query_point: the solved p, which lies beside a q that query_solve admitted).
template <bool kClamp>
OW_DEV SurfaceSample sample_point_in(const u16x4 *disp, const u16x4 *norm, int n, int cascades, const SurfaceScales &scales, float x, float z) {
    float dsum[3] = {0.0f, 0.0f, 0.0f}, g[2] = {0.0f, 0.0f}, gs[2] = {0.0f, 0.0f}, foam = 0.0f;
    float gf[2] = {0.0f, 0.0f}, foam_f = 0.0f;
    const size_t plane = (size_t)n * n;
    for (int c = 0; c < cascades; ++c) {
        const float sx = scales.s[c][0], sy = scales.s[c][1], sz = scales.s[c][2], sw = scales.s[c][3];
        const float u = kClamp ? clamp_coord(x * sx) : x * sx, v = kClamp ? clamp_coord(z * sy) : z * sy;
        const Tap t = make_tap(u, v, n);
        float d[4], m[4];
        bilinear(disp + c * plane, n, t, d);
        bilinear(norm + c * plane, n, t, m);
        for (int k = 0; k < 3; ++k) dsum[k] += d[k] * sz;
        g[0] += m[0];
        g[1] += m[1];
        gs[0] += m[0] * sw;
        gs[1] += m[1] * sw;
        foam += m[3];
        {   // water.gdshader:74-82 fragment(): bicubic and bilinear mixed by the pixels per metre of this cascade
            float bc[4];
            const float ppm = (float)n * fminf(sx, sy);
            const float a = fminf(1.0f, ppm * 0.1f);
            bicubic(norm + c * plane, n, u, v, bc);
            gf[0] += glsl_mix(bc[0], m[0], a) * sw;
            gf[1] += glsl_mix(bc[1], m[1], a) * sw;
            foam_f += glsl_mix(bc[3], m[3], a) * 1.0f;
        }
    }
    // sea_spray_particle.gdshader:83-89
    const float normal_y = 1.0f / sqrtf(g[0] * g[0] + 1.0f + g[1] * g[1]);
    const float normal_factor = glsl_mix(0.25f, 1.0f, fminf((normal_y - 0.92f) / (0.99f - 0.92f), 1.0f));
    const float foam_factor = glsl_mix(0.25f, 1.0f, fminf((foam - 0.9f) / (1.0f - 0.9f), 1.0f));
    SurfaceSample s;
    s.displacement[0] = dsum[0];
    s.displacement[1] = dsum[1];
    s.displacement[2] = dsum[2];
    s.gradient[0] = g[0];
    s.gradient[1] = g[1];
    s.gradient_scaled[0] = gs[0];
    s.gradient_scaled[1] = gs[1];
    s.foam = foam;
    s.normal_factor = normal_factor;
    s.foam_factor = foam_factor;
    s.scale_factor = normal_factor * foam_factor;
    s.spray_active = (normal_factor >= 0.0f && normal_factor <= 1.0f && foam > 0.9f) ? 1 : 0;
    s.gradient_fragment[0] = gf[0];
    s.gradient_fragment[1] = gf[1];
    s.foam_fragment = foam_f;
    s.reserved = 0.0f;
    return s;
}
// k_sample_surface's per-point body: finite in every field for any (x, z)
OW_DEV SurfaceSample sample_point(const u16x4 *disp, const u16x4 *norm, int n, int cascades, const SurfaceScales &scales, float x, float z) {
    return sample_point_in<true>(disp, norm, n, cascades, scales, x, z);
}

// ---- the inverse query: where is the water above (x, z)? ----------------------------------------------------------------------------

// e^a for a <= 0 in the four basic operations: a = k ln2 + r (Cody-Waite, |r| <= ln2 / 2), e^r by its degree-7 Taylor polynomial
// (truncation below 2e-9 relative), 2^k built in the exponent field.  Relative error a few ulp; 0 below -87 (where 2^k leaves the
// normal range).  The same bits on the device and on the host.
OW_DEV float exp_f32(float a) {
    if (!(a > -87.0f)) return 0.0f;
    const float k = floorf(a * 1.44269504f + 0.5f);
    const float r = (a - k * 0.693145752f) - k * 1.42860677e-6f;
    float p = 1.98412698e-4f;
    p = p * r + 1.38888889e-3f;
    p = p * r + 8.33333333e-3f;
    p = p * r + 4.16666667e-2f;
    p = p * r + 1.66666667e-1f;
    p = p * r + 0.5f;
    p = p * r + 1.0f;
    p = p * r + 1.0f;
    const uint32_t bits = (uint32_t)((int)k + 127) << 23;
    float scale;
    __builtin_memcpy(&scale, &bits, 4);
    return p * scale;
}

// water.gdshader:29: f = min(exp(-(|p - c| - 150) * 0.007), 1) and its gradient df/dp (zero inside 150 m, where f is the constant 1)
OW_DEV float falloff_at(const QueryParams &qp, float x, float z, float grad[2]) {
    grad[0] = grad[1] = 0.0f;
    if (!qp.falloff) return 1.0f;
    const float dx = x - qp.center[0], dz = z - qp.center[1];
    const float dist = sqrtf(dx * dx + dz * dz);
    const float a = -(dist - 150.0f) * 0.007f;
    if (!(a < 0.0f)) return 1.0f;
    const float f = exp_f32(a);
    if (dist > 0.0f) {
        const float s = f * -0.007f / dist;
        grad[0] = s * dx;
        grad[1] = s * dz;
    }
    return f;
}

// The displacement sum's horizontal part S(p) = sum_i D_xz,i(p) (water.gdshader:31-37, the .x and .z of the sum sample_point
// forms, in the same operations) and its Jacobian dS[k][j] = dS_k / dp_j: the derivative of each cascade's bilinear interpolant
// inside its cell, from the same four texels the lookup loads.
OW_DEV void displacement_xz(const u16x4 *disp, int n, int cascades, const SurfaceScales &scales, float x, float z, float S[2], float dS[2][2]) {
    S[0] = S[1] = 0.0f;
    dS[0][0] = dS[0][1] = dS[1][0] = dS[1][1] = 0.0f;
    const size_t plane = (size_t)n * n;
    for (int c = 0; c < cascades; ++c) {
        const float sx = scales.s[c][0], sy = scales.s[c][1], sz = scales.s[c][2];
        const Tap t = make_tap(x * sx, z * sy, n);
        float a[4], b[4], cc[4], d[4];
        load_quad(disp + c * plane, n, t, a, b, cc, d);
        const float ux = 1.0f - t.wx, uy = 1.0f - t.wy;
        const float kx = (float)n * sx * sz, kz = (float)n * sy * sz;  // d(weight)/d(world) times the cascade's scale
        for (int j = 0; j < 2; ++j) {
            const int ch = 2 * j;  // .x and .z
            const float top = a[ch] * ux + b[ch] * t.wx, bot = cc[ch] * ux + d[ch] * t.wx;
            S[j] += (top * uy + bot * t.wy) * sz;
            dS[j][0] += ((b[ch] - a[ch]) * uy + (d[ch] - cc[ch]) * t.wy) * kx;
            dS[j][1] += (bot - top) * kz;
        }
    }
}

// F(p) = p + f(p) S(p) - q, its Jacobian, f(p) and |F| (a non-finite |F| counts as the largest float: it never wins a comparison)
struct QueryEval {
    float F[2], J[2][2], f, r;
};
OW_DEV QueryEval query_eval(const u16x4 *disp, int n, int cascades, const SurfaceScales &scales, const QueryParams &qp, float px, float pz,
                            float qx, float qz) {
    float S[2], dS[2][2], gf[2];
    displacement_xz(disp, n, cascades, scales, px, pz, S, dS);
    QueryEval e;
    e.f = falloff_at(qp, px, pz, gf);
    e.F[0] = (px + e.f * S[0]) - qx;
    e.F[1] = (pz + e.f * S[1]) - qz;
    for (int k = 0; k < 2; ++k)
        for (int j = 0; j < 2; ++j) e.J[k][j] = (k == j ? 1.0f : 0.0f) + e.f * dS[k][j] + S[k] * gf[j];
    const float r = sqrtf(e.F[0] * e.F[0] + e.F[1] * e.F[1]);
    e.r = (r <= 3.0e38f) ? r : 3.4028235e38f;
    return e;
}

// Damped Newton on F(p) = 0 from p = q.  Each step is searched by halving (at most kQueryBacktracks times) until |F| decreases.  Where
// det J <= kQueryDetMin -- a crest where the sheet folds over, or about to -- and wherever the Newton step finds no decrease, the step
// is the fixed-point step -F instead (p <- q - f(p) D(p): the Newton step with J taken as the identity, a descent direction wherever
// the map does not fold).  Only decreases are accepted, so the iterate held is the one of smallest |F| so far; the loop ends at the
// tolerance, after max_iterations, or when neither step decreases |F|.  converged = that |F| is within the tolerance.  A non-finite q
// (or one beyond 3e38, or beyond kCoordMax tiles of a cascade) gives p = (0, 0), converged = 0: no q puts a NaN or an Inf in a record.
//
// On the demo scene (cascades 0-2 at 1024^2, two ticks, q uniform in [-500, 500]^2) 97.4 % of points converge to 1e-3 m with the
// defaults, after 5.6 iterations and 7.7 evaluations of F on average (tests/test_surface_query.py); the misses sit on folded crests.
constexpr int kQueryBacktracks = 6;
constexpr float kQueryDetMin = 0.1f;
// one damped step along (sx, sz): halve until |F| decreases; false if it never does
OW_DEV bool query_line_search(const u16x4 *disp, int n, int cascades, const SurfaceScales &scales, const QueryParams &qp, float qx, float qz,
                              float sx, float sz, float &px, float &pz, QueryEval &e, int &evals) {
    float step = 1.0f;
    for (int b = 0; b <= kQueryBacktracks; ++b, step *= 0.5f) {
        const float nx = px + step * sx, nz = pz + step * sz;
        const QueryEval en = query_eval(disp, n, cascades, scales, qp, nx, nz, qx, qz);
        ++evals;
        if (en.r < e.r) {
            px = nx;
            pz = nz;
            e = en;
            return true;
        }
    }
    return false;
}
// The Newton loop of query_point from a given start p0 (query_point: p0 = q; the buoyancy kernel's warm start: the previous step's p
// moved with q).  A non-finite q (or one beyond 3e38 or kCoordMax tiles) gives p = (0, 0) and no iteration; p0 must be finite.
struct QuerySolution {
    float p[2];
    QueryEval e;  // F at p
    int iterations, evaluations;
    bool finite;  // q was finite: converged = finite && e.r <= tolerance
};
OW_DEV QuerySolution query_solve(const u16x4 *disp, int n, int cascades, const SurfaceScales &scales, const QueryParams &qp, float qx, float qz,
                                 float p0x, float p0z) {
    bool finite = fabsf(qx) <= 3.0e38f && fabsf(qz) <= 3.0e38f;
    for (int c = 0; c < cascades; ++c)  // ... or whose texture coordinate in some cascade is beyond kCoordMax
        finite = finite && fabsf(qx * scales.s[c][0]) <= kCoordMax && fabsf(qz * scales.s[c][1]) <= kCoordMax;
    float px = finite ? p0x : 0.0f, pz = finite ? p0z : 0.0f;
    QueryEval e = query_eval(disp, n, cascades, scales, qp, px, pz, qx, qz);
    int it = 0, evals = 1;
    if (finite) {
        for (; it < qp.max_iterations && e.r > qp.tolerance; ++it) {
            const float det = e.J[0][0] * e.J[1][1] - e.J[0][1] * e.J[1][0];
            bool moved = false;
            if (det > kQueryDetMin) {
                const float sx = (e.J[0][1] * e.F[1] - e.J[1][1] * e.F[0]) / det;
                const float sz = (e.J[1][0] * e.F[0] - e.J[0][0] * e.F[1]) / det;
                moved = query_line_search(disp, n, cascades, scales, qp, qx, qz, sx, sz, px, pz, e, evals);
            }
            if (!moved) moved = query_line_search(disp, n, cascades, scales, qp, qx, qz, -e.F[0], -e.F[1], px, pz, e, evals);
            if (!moved) {  // |F| is at a local minimum above the tolerance (a fold), or the steps are below float resolution
                ++it;
                break;
            }
        }
    }
    QuerySolution sol;
    sol.p[0] = px;
    sol.p[1] = pz;
    sol.e = e;
    sol.iterations = it;
    sol.evaluations = evals;
    sol.finite = finite;
    return sol;
}

OW_DEV SurfaceQuery query_point(const u16x4 *disp, const u16x4 *norm, int n, int cascades, const SurfaceScales &scales, const QueryParams &qp,
                                float qx, float qz) {
    SurfaceQuery out;
    out.world_xz[0] = qx;
    out.world_xz[1] = qz;
    out.reserved[0] = out.reserved[1] = out.reserved[2] = 0;
    const QuerySolution sol = query_solve(disp, n, cascades, scales, qp, qx, qz, qx, qz);
    const float px = sol.p[0], pz = sol.p[1];
    const QueryEval &e = sol.e;
    const int it = sol.iterations, evals = sol.evaluations;
    const bool finite = sol.finite;
    out.p[0] = px;
    out.p[1] = pz;
    out.residual = e.r;
    out.iterations = it;
    out.evaluations = evals;
    out.converged = (finite && e.r <= qp.tolerance) ? 1 : 0;
    out.falloff = e.f;
    out.sample = sample_point_in<false>(disp, norm, n, cascades, scales, px, pz);
    out.height = e.f * out.sample.displacement[1];
    // water.gdshader:83,90: normalize(vec3(-gradient.x, 1, -gradient.y)) of the bilinear scaled gradient
    const float gx = out.sample.gradient_scaled[0], gz = out.sample.gradient_scaled[1];
    const float inv = 1.0f / sqrtf(gx * gx + 1.0f + gz * gz);
    out.normal[0] = -gx * inv;
    out.normal[1] = inv;
    out.normal[2] = -gz * inv;
    return out;
}

}  // namespace ow
